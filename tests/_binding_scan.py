"""A scan of a built CircuitBuilder circuit for witness cells that no constraint binds: the outer circuits' counterpart of
tests/test_oracle_soundness.py::test_every_main_column_is_constrained_on_some_row.  CPU only; nothing here imports the device library.

One description (programs, generators, cycles, schedule) feeds the replay, the oracle, the device and both verifiers, so a constraint a
builder forgot is invisible to every word-for-word test.  The scan asks the constraints themselves, through the C entry behind
_oracle.plonk_gate_constraints_base (the circuit struct built once per subject), on the honest witness of tests/_witness_reading.replay.

  Subject           a circuit with its constants, partial witness, public-input hash and honest witness
  written_cells     the cells a generator or a scheduled copy writes: the non-input cells that end EQUAL in two replays over partial
                    witnesses whose non-input cells hold different random fillings (`honest != partial` alone misses generated zeros)
  class_scan        classes = the sets of c.cycles, every other cell a singleton.  Every class that holds a written cell, an input cell
                    or more than one cell has ALL its cells set to v + 1, then to v + 0x123456789abcdef: it is BOUND if a touched row
                    becomes non-zero under either value, else SILENT.  A looking or table row has no gate constraint and is judged by the
                    lookup reading (tests/_lookup_tables_cases.py over tests/_lookup_cases.py): bound if a looked-up pair is absent from
                    its table or a term of the argument stops vanishing.
                    Beyond that, a class whose cell a GENERATOR writes on a row of a gate with constraints is UNDEFINED if that row stays
                    zero while only consumers object: the consumers then say "consistent", nobody says "computed".  (This is what a
                    dropped output-defining constraint looks like when the output is wired on: the consumers still bind the class.)
  judge             one class under both values: the verdict the scans and tests/test_gpu_circuit_binding.py share
  Subject.mute      rows the honest witness leaves unsatisfied (only the synthetic many-generators circuit has any): never asked, and
                    the classes that touch them are not scanned
  resplit_scan      two rows per gate with constraints; on each, every ordered pair (i, j) of wires the gate's constraints read is moved by
                    (+B, -1) and (-B, +1), B in 2, 4, 2^16, 2^32: the row must become non-zero.  This is what a missing range or
                    booleanity constraint looks like, which no one-cell flip shows.  A gate that reads more than 80 wires: one row, B in
                    2, 2^32.  Row level only: wiring is the "cells hold the reading's values" tests'.
  drop_constraint   a copy of a circuit description with one constraint taken out of the program words (the planted holes)
  readings_for_test_circuits, blind_rows
                    the readings of kinds 1 and 17 for the replay of the lookup and blinding test circuits, registered for a block, and
                    the blinding rows (kind 18), filled before anything else runs as on the device"""
import contextlib
import ctypes as C
import time

import numpy as np

from tests import _lookup_tables_cases as ltc
from tests import _merkle_reading as mr
from tests import _oracle
from tests import _witness_reading as rd

P = _oracle.P
DELTAS = (1, 0x123456789abcdef)
RESPLIT_B = (2, 4, 1 << 16, 1 << 32)
WIDE_GATE = 80                                                  # read wires above which a gate gets one row and B in 2, 2^32
LOOKUP_D, LOOKUP_ETAS, LOOKUP_THETAS = 8, [5, 1 << 40], [P - 3, 77]


# ---- readings the test circuits need beyond tests/_witness_reading.py ------------------------------------------------------------------
def _arithmetic_row(w, n_ops, c0, c1):
    for k in range(n_ops):
        w[4 * k + 3] = (c0 * w[4 * k] * w[4 * k + 1] + c1 * w[4 * k + 2]) % P


@contextlib.contextmanager
def readings_for_test_circuits():
    """kinds 1 (SIPP_GEN_ARITHMETIC), 17 (SIPP_GEN_LOOKUP, tests/_lookup_tables_cases.generate) and 18 (SIPP_GEN_RANDOM: nothing, see
    blind_rows) in rd.READINGS while the block runs"""
    from tests import _blinding_cases as bc

    def lookup(wires, consts, pih, p, rows):
        gate = int(consts[_sel_of[0], rows[0]])
        wires[:] = ltc.generate(wires, consts, [(ltc.GEN_LOOKUP, _sel_of[0], gate) + tuple(p)], [int(r) for r in rows])[0]

    def random(wires, consts, pih, p, rows):
        pass                                                    # blind_rows() has filled them before anything else ran, as the device does

    # run_generator hands a reading the parameters but not the selector column: the wrapper below notes it
    _sel_of = [0]
    saved_run, saved = rd.run_generator, dict(rd.READINGS)

    def run_generator(wires, consts, pih, g, rows):
        _sel_of[0] = g[1]
        return saved_run(wires, consts, pih, g, rows)
    rd.READINGS.update({rd.GEN_ARITHMETIC: rd._row_by_row(lambda w, p, c: _arithmetic_row(w, p[0], c(p[1]), c(p[2]))),
                        ltc.GEN_LOOKUP: lookup, bc.GEN_RANDOM: random})
    rd.run_generator = run_generator
    try:
        yield
    finally:
        rd.run_generator = saved_run
        rd.READINGS.clear()
        rd.READINGS.update(saved)


_blind = {}


def blind_rows(c, consts):
    """(values, mask) of the blinding rows (SIPP_GEN_RANDOM under tests/_blinding_cases.SEED, counter 0), read once a circuit: the
    device fills them before anything else runs, so the scheduled copies into a pair's second row land on top of them"""
    from tests import _blinding_cases as bc
    if id(c) not in _blind:
        gens = [g for g in c.generators() if g[0] == bc.GEN_RANDOM]
        _blind[id(c)] = bc.blind_fill(np.zeros((c.num_wires, c.n), dtype=np.uint64), consts, gens, bc.SEED, 0) if gens else None
    return _blind[id(c)]


# ---- the subject -----------------------------------------------------------------------------------------------------------------------
class _Rows:
    """orc_plonk_gate_constraints_base (the entry behind _oracle.plonk_gate_constraints_base) on one row at a time.  A row is judged by
    a description that keeps only the gate the row holds: every other gate's filter vanishes on the row, so the verdict is the whole
    circuit's, without evaluating the Poseidon gate's 123 constraints on every row.  Structs and row-major constants are built once."""

    def __init__(self, circ, consts, pih, gate_of_row):
        self.L = _oracle._plonk_gates_lib()
        self.circ, self.gate_of_row, self.sub = circ, gate_of_row, {}
        self.kT = np.ascontiguousarray(np.asarray(consts, dtype=np.uint64).T)
        self.pih = np.asarray([int(x) for x in pih], dtype=np.uint64)
        self.out = np.zeros(max(1, circ["num_gate_constraints"]), dtype=np.uint64)

    def nonzero(self, row_wires, r):
        g = int(self.gate_of_row[r])
        if self.circ["gates"][g][5] == 0:
            return False
        if g not in self.sub:
            self.sub[g] = _oracle.plonk_circuit(dict(self.circ, gates=[self.circ["gates"][g]]))
        self.out[:] = 0
        self.L.orc_plonk_gate_constraints_base(C.byref(self.sub[g]), row_wires, self.kT[r], self.pih, self.out)
        return bool(self.out.any())


class Subject:
    """c: the built circuit; cs: its constants_sigmas; partial: the partial witness of the honest inputs; pih: the public inputs'
    hash; honest: the replayed witness (replayed here if None); circ: another description to judge by (a planted hole)"""

    def __init__(self, name, c, cs, partial, pih, honest=None, circ=None, written=None):
        self.name, self.c, self.n, self.pih, self.written_override = name, c, c.n, [int(x) for x in pih], written
        self.circ = c.circuit() if circ is None else circ
        self.consts = np.ascontiguousarray(cs[:c.num_constants])
        self.partial = np.ascontiguousarray(partial, dtype=np.uint64)
        self.honest = self.replay(self.partial) if honest is None else honest
        self.replayed = self.honest                             # before the multiplicities, which no generator writes
        self.desc = tuple(int(x) for x in self.circ.get("lookup", (0,) * 8))
        self.gate = np.asarray(c.gate)
        self.rows = _Rows(self.circ, self.consts, self.pih, self.gate)
        self.constrained = np.array([g[5] > 0 for g in self.circ["gates"]])[self.gate]          # per row: its gate has constraints
        self.lookup_row = np.zeros(self.n, dtype=bool)
        if any(self.desc):
            self.lookup_row = (self.consts[self.desc[0]] != 0) | (self.consts[self.desc[3]] != 0)
            self._lookup_setup()
        self.wT = np.ascontiguousarray(self.honest.T)           # [row][wire]: a row's wires are contiguous
        inputs = np.zeros(c.num_wires * c.n, dtype=bool)
        for cyc in list(c.pi_cycle) + list(c.in_cycle):
            inputs[np.asarray(cyc, dtype=np.int64)] = True
        if written is None:
            inputs |= self.partial.reshape(-1) != 0
        self.mute = set()                                       # rows the honest witness does not satisfy (set by the caller): never heard
        self.inputs = inputs                                    # as far as the description tells: written_cells() takes out what is generated

    def replay(self, partial):
        c = self.c
        blind = blind_rows(c, self.consts)
        if blind is not None:
            partial = partial.copy()
            partial[blind[1]] = blind[0][blind[1]]
        return rd.replay(partial, self.consts, c.generators(), self.pih, c.schedule())

    def unsatisfied_rows(self):
        return [r for r in range(self.n) if not self.lookup_row[r] and self.rows.nonzero(self.wT[r], r)]

    # ---- lookups ----
    def _lookup_setup(self):
        """the honest table with its multiplicities, the running sums under fixed challenges, and the set of (tag, x, y) entries"""
        d, k = self.desc, self.consts
        self.honest = ltc.multiplicities(d, self.honest, k)
        self.cols, closes = ltc.sums(d, self.honest, k, LOOKUP_D, LOOKUP_ETAS, LOOKUP_THETAS)
        assert closes
        self.entries = set()
        for i in np.flatnonzero(k[d[3]]):
            tag = ltc.row_tags(d, k, i)[1]
            for s in range(d[6]):
                self.entries.add((tag, int(k[d[4] + 2 * s][i]) % P, int(k[d[4] + 2 * s + 1][i]) % P))

    def lookup_objects(self, r):
        """whether the lookup reading refuses row r of the table as it stands: a looked-up pair in no table, or a term that stops
        vanishing under the honest running sums"""
        d, k, wires = self.desc, self.consts, self.wT.T
        if int(k[d[0]][r]) % P:
            tag = ltc.row_tags(d, k, r)[0]
            for s in range(d[2]):
                if (tag, int(wires[d[1] + 2 * s][r]) % P, int(wires[d[1] + 2 * s + 1][r]) % P) not in self.entries:
                    return True
        return any(t for c in range(len(LOOKUP_ETAS))
                   for t in ltc.terms_on_row(d, wires, k, LOOKUP_D, self.cols, len(LOOKUP_ETAS), c, LOOKUP_ETAS[c], LOOKUP_THETAS[c], r))

    def objects(self, r):
        if r in self.mute:
            return False
        return self.lookup_objects(r) if self.lookup_row[r] else self.rows.nonzero(self.wT[r], r)


# ---- written cells, classes ------------------------------------------------------------------------------------------------------------
def written_cells(s, seed=20261):
    """-> (written, by a copy, input): boolean masks over the flat cells.  A cell on a public input's cycle that the partial witness
    leaves at zero and a generator fills (an output that is public) counts as written, not as input."""
    copied = np.zeros(s.partial.size, dtype=bool)
    copied[s.c.schedule()["copy_dst"].astype(np.int64)] = True
    if s.written_override is not None:
        written = s.written_override.reshape(-1)
        return written, copied & written, s.inputs & ~written
    fills = []
    for k in range(2):
        rng = np.random.default_rng(seed + k)
        flat = s.partial.reshape(-1).copy()
        fill = _oracle.rand_field(rng, flat.shape)
        flat[~s.inputs] = fill[~s.inputs]
        fills.append(s.replay(flat.reshape(s.partial.shape)).reshape(-1))
    changed = s.replayed.reshape(-1) != s.partial.reshape(-1)
    written = (fills[0] == fills[1]) & (~s.inputs | changed)
    # a generator that read a cell nobody writes would differ between the replays and hide what it wrote: nothing may be missed
    missed = changed & ~written
    assert not missed.any(), ("cells the honest replay changes but the two fillings disagree on", np.flatnonzero(missed)[:8])
    return written, copied & written, s.inputs & ~written


def classes(s, written, inputs):
    """the classes the scan flips: every cycle, and every written or input cell outside the cycles as a singleton"""
    on_cycle = np.zeros(len(written), dtype=bool)
    out = []
    for cyc in s.c.cycles:
        a = np.asarray(cyc, dtype=np.int64)
        on_cycle[a] = True
        out.append(a)
    out += [np.array([x], dtype=np.int64) for x in np.flatnonzero((written | inputs) & ~on_cycle)]
    return out


def judge(s, cls, generated):
    """one class under both values -> "bound", "silent" or "undefined" (see the module's docstring); the table is left as it was"""
    n, wT = s.n, s.wT
    rows, wires = cls % n, cls // n
    vals = wT[rows, wires]
    v = int(vals[0])
    assert (vals == vals[0]).all(), "the honest witness breaks a cycle"
    touched = sorted(set(rows.tolist()))
    own = sorted({int(x % n) for x in cls[generated[cls]] if s.constrained[x % n]})             # rows whose generator wrote a cell of the class
    objecting = set()
    try:
        for d in DELTAS:
            wT[rows, wires] = np.uint64((v + d) % P)
            for r in own + [r for r in touched if r not in own]:
                if r not in objecting and s.objects(r):
                    objecting.add(r)
                    if not own or set(own) <= objecting:
                        break
            if objecting and set(own) <= objecting:
                break
    finally:
        wT[rows, wires] = np.uint64(v)
    return "silent" if not objecting else "bound" if set(own) <= objecting else "undefined"


def class_scan(s, only_rows=None):
    """-> {"silent": [...], "undefined": [...], "scanned": mask of the cells in scanned classes, "classes": count, "seconds": ...}; an
    item is the tuple of a class's flat cells.  only_rows: scan only the classes that touch one of these rows"""
    t0 = time.time()
    written, copied, inputs = written_cells(s)
    generated = written & ~copied
    out = {"silent": [], "undefined": [], "scanned": np.zeros(len(written), dtype=bool), "classes": 0, "skipped": 0}
    for cls in classes(s, written, inputs):
        rows = set((cls % s.n).tolist())
        if only_rows is not None and not rows & set(only_rows):
            continue
        if s.mute and rows & s.mute:                            # a row that was never satisfied cannot be asked
            out["skipped"] += 1
            continue
        out["classes"] += 1
        out["scanned"][cls] = True
        verdict = judge(s, cls, generated)
        if verdict != "bound":
            out[verdict].append(tuple(int(x) for x in cls))
    out["seconds"] = time.time() - t0
    return out


# ---- the re-split scan -----------------------------------------------------------------------------------------------------------------
def read_wires(circ, gate):
    _, _, _, _, off, nc = circ["gates"][gate]
    return sorted({idx for cons in mr.decode(circ["programs"], off, nc) for _, f in cons for kind, idx in f if kind == 0})


def resplit_rows(s, rows_per_gate=2):
    """{gate: its rows to scan}: the first and the last row that holds the gate (one row for a wide gate)"""
    out = {}
    for g, gt in enumerate(s.circ["gates"]):
        held = np.array([r for r in np.flatnonzero(s.gate == g) if r not in s.mute], dtype=np.int64)
        if gt[5] == 0 or not len(held):
            continue
        wide = len(read_wires(s.circ, g)) > WIDE_GATE
        pick = [int(held[0]), int(held[-1])][:1 if wide else rows_per_gate]
        out[g] = sorted(set(pick))
    return out


def resplit_scan(s, rows_per_gate=2, only_rows=None):
    """-> {"silent": [(gate, row, i, j, B, sign)], "pairs": count, "seconds": ...}: sign +1 is (w_i + B, w_j - 1), -1 is (w_i - B, w_j + 1)"""
    t0 = time.time()
    silent, count = [], 0
    for g, rows in resplit_rows(s, rows_per_gate).items():
        reads = read_wires(s.circ, g)
        bs = (2, 1 << 32) if len(reads) > WIDE_GATE else RESPLIT_B
        for r in rows:
            if only_rows is not None and r not in only_rows:
                continue
            base = s.wT[r].copy()
            assert not s.rows.nonzero(base, r), "the honest row is not satisfied"
            row = base.copy()
            for i in reads:
                for j in reads:
                    if i == j:
                        continue
                    count += 1
                    vi, vj = int(base[i]), int(base[j])
                    for B in bs:
                        for sign in (1, -1):
                            row[i], row[j] = (vi + sign * B) % P, (vj - sign) % P
                            if not s.rows.nonzero(row, r):
                                silent.append((g, r, i, j, B, sign))
                    row[i], row[j] = vi, vj
    return {"silent": silent, "pairs": count, "seconds": time.time() - t0}


# ---- planted holes -----------------------------------------------------------------------------------------------------------------------
def drop_constraint(circ, gate, which):
    """a copy of the description with constraint `which` of `gate` taken out of the program words; every gate keeps its other words"""
    prog = [int(x) for x in circ["programs"]]
    words, gates = [], []
    for g, (si, row, lo, hi, off, nc) in enumerate(circ["gates"]):
        at, start, kept = off, len(words), 0
        for j in range(nc):
            end = at + 1
            for _ in range(prog[at]):
                end += 2 + 2 * prog[end + 1]
            if (g, j) != (gate, which):
                words += prog[at:end]
                kept += 1
            at = end
        gates.append((si, row, lo, hi, start, kept))
    out = dict(circ)
    out.update(gates=gates, programs=np.array(words, dtype=np.int64), num_gate_constraints=max(g[5] for g in gates))
    return out


def cell(s, wire, row):
    return wire * s.n + row
