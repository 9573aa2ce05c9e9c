"""A catalogue of gate sets at the edges of the outer prover's gate programs (sipp_plonk_prove_gates, "SIPPPLK3"): the shapes the
compiled quotient (compile_gates / plonk_quotient_kernel in sipp_amd/csrc/plonk.hip) and both verifiers must read exactly as written, built
explicitly rather than drawn at random.

A circuit is the dict tools/plonk_synth.circuit() returns (num_wires, num_routed, num_constants, num_selectors, gates =
[(selector_index, row, group_lo, group_hi, prog_offset, num_constraints)], programs, num_gate_constraints).  Every constraint is written as
poly(inputs) - out with `out` a wire that no polynomial of its gate reads; the witness fills every input cell with edge values (0, 1,
p - 1, 2^32 - 1, 2^32, p - 2^32) and random ones and computes each `out` with Python integers mod p, so the SATISFIED entries are
satisfied on every row.  The second class (accept=False) is over-degree (64-factor monomials, a 64-gate selector group) or tampered
after the witness was computed: every verifier must refuse its proof at the quotient identity.

Each entry function returns a dict: name, circ, num_routed, num_challenges, log_n, wires [num_wires][N], cs (constants then sigmas,
[num_constants + num_routed][N]), pis, pih, gate (the gate of every row), satisfied, bad_rows (rows whose constraints do not vanish),
accept (whether every verifier must accept its proof)."""
import functools

import numpy as np

from tests import _oracle

P = _oracle.P
UNUSED = (1 << 32) - 1
W, K, PIH = 0, 1, 2
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EDGE_VALUES = (0, 1, P - 1, (1 << 32) - 1, 1 << 32, P - (1 << 32))
EDGE_COEFS = (0, 1, -1, (1 << 32) - 1, -((1 << 32) - 1), 1 << 32, -(1 << 32), I64_MAX, I64_MIN)
MAX_DEGREE = 8                      # filter degree + monomial degree, rate_bits = 3
LOG_N = 10                          # the smallest trace the device prover takes (its FRI: 10 .. 24 degree bits)
FRI = dict(rate_bits=3, cap_height=1, nq=4, arity=4, fpb=3)
DIGEST = (17, 0, P - 1, 1 << 32)


class Builder:
    """gate programs in the word layout of sipp_plonk_circuit: per constraint n_mono, then per monomial coef, n_factors, (kind, index)..."""

    def __init__(self):
        self.prog, self.gates, self.specs = [], [], []

    def gate(self, sel, row, lo, hi, constraints):
        """constraints: [(monos, out)]: monos = [(coef, [(kind, index), ...])], out = the output wire (a -1 monomial) or None"""
        off = len(self.prog)
        for monos, out in constraints:
            ms = list(monos) + ([(-1, [(W, out)])] if out is not None else [])
            self.prog.append(len(ms))
            for coef, fs in ms:
                self.prog += [coef, len(fs)]
                for kind, idx in fs:
                    self.prog += [kind, idx]
        outs = [out for _, out in constraints if out is not None]
        read = {(k, i) for monos, _ in constraints for _, fs in monos for k, i in fs}
        assert len(set(outs)) == len(outs) and not any((W, o) in read for o in outs), "an output wire is read by its own gate"
        self.gates.append((sel, row, lo, hi, off, len(constraints)))
        self.specs.append(constraints)

    def circuit(self, num_wires, num_routed, num_constants, num_selectors):
        return {"num_wires": num_wires, "num_routed": num_routed, "num_constants": num_constants, "num_selectors": num_selectors,
                "gates": list(self.gates), "programs": np.array(self.prog, dtype=np.int64),
                "num_gate_constraints": max(g[5] for g in self.gates)}


def _operand(kind, idx, wires, consts, pih):
    return wires[idx] if kind == W else consts[idx] if kind == K else pih[idx]


def _poly(monos, wires, consts, pih):
    s = 0
    for coef, fs in monos:
        t = coef % P
        for kind, idx in fs:
            t = t * int(_operand(kind, idx, wires, consts, pih)) % P
        s = (s + t) % P
    return s


def eval_row_exact(circ, wires, consts, pih):
    """evaluate_gate_constraints over the integers mod p, straight from the program words: term_j = sum_g filter_g(s) constraint_(g, j);
    wires / consts: one row (ints)"""
    prog = [int(x) for x in circ["programs"]]
    out = [0] * circ["num_gate_constraints"]
    for (sel, row, lo, hi, off, nc) in circ["gates"]:
        s = int(consts[sel])
        f = 1
        for i in range(lo, hi):
            if i != row:
                f = f * (i - s) % P
        if circ["num_selectors"] > 1:
            f = f * (UNUSED - s) % P
        w = off
        for j in range(nc):
            nm = prog[w]
            w += 1
            acc = 0
            for _ in range(nm):
                t, nf = prog[w] % P, prog[w + 1]
                w += 2
                for _f in range(nf):
                    t = t * int(_operand(prog[w], prog[w + 1], wires, consts, pih)) % P
                    w += 2
                acc = (acc + t) % P
            out[j] = (out[j] + f * acc) % P
    return out


def _merged(monos):
    """the same polynomial with equal factor multisets summed (exact over the integers mod p): fewer products per row"""
    acc = {}
    for coef, fs in monos:
        key = tuple(sorted(fs))
        acc[key] = (acc.get(key, 0) + coef) % P
    return [(c, list(f)) for f, c in acc.items()]


def _fill(rng, rows, n, base):
    """uniform field elements with an edge value in every third cell (by column and row)"""
    a, r = np.indices((rows, n))
    edge = np.array(EDGE_VALUES, dtype=np.uint64)[(3 * (a + base) + r) % len(EDGE_VALUES)]
    return np.where((a + base + 2 * r) % 3 == 0, edge, _oracle.rand_field(rng, (rows, n))).astype(np.uint64)


def _witness(b, circ, seed, row_gates, pis, cycles=0, tamper=None, C=2, name="", over_degree=False):
    """fill the table: selectors name the row's gate, every other constant and wire is an input (edge or random), routed input cells
    optionally joined in 3-cycles of the wire permutation, then every output of the row's gate from its polynomial"""
    rng = np.random.default_rng(seed)
    n, Wn, R, Kn, S = 1 << LOG_N, circ["num_wires"], circ["num_routed"], circ["num_constants"], circ["num_selectors"]
    pih = [int(x) for x in _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))]
    gate = np.array([row_gates[r % len(row_gates)] for r in range(n)], dtype=np.int64)
    wires, consts = _fill(rng, Wn, n, 0), _fill(rng, Kn, n, 100)
    gsel = np.array([g[0] for g in circ["gates"]])[gate]
    grow = np.array([g[1] for g in circ["gates"]], dtype=np.uint64)[gate]
    for s in range(S):
        consts[s] = np.where(gsel == s, grow, np.uint64(UNUSED))
    assert S > 1 or (consts[0] != UNUSED).all()
    outs = [{o for _, o in spec if o is not None} for spec in b.specs]
    perm = np.arange(R * n)
    if cycles:
        free = [j * n + r for j in range(R) for r in range(n) if j not in outs[gate[r]]]
        order = np.array(free)[rng.permutation(len(free))][:3 * cycles]
        flat = wires[:R].reshape(-1)                                                  # a view: writes go into the table
        for q in range(0, len(order) - 2, 3):
            x, y, z = order[q:q + 3]
            perm[x], perm[y], perm[z] = y, z, x
            flat[y] = flat[z] = flat[x]
    progs = [[(_merged(monos), o) for monos, o in spec if o is not None] for spec in b.specs]
    for r in range(n):
        col_w, col_c = wires[:, r], consts[:, r]
        for monos, o in progs[gate[r]]:
            wires[o, r] = _poly(monos, col_w, col_c, pih)
    bad_rows = set()
    if tamper is not None:
        j, r = tamper
        wires[j, r] = (int(wires[j, r]) + 1) % P
        bad_rows.add(r)
    w = pow(7, (P - 1) >> LOG_N, P)
    pw, ks = [pow(w, i, P) for i in range(n)], [pow(7, j, P) for j in range(R)]
    sig = np.array([[ks[int(q) // n] * pw[int(q) % n] % P for q in perm[j * n:(j + 1) * n]] for j in range(R)], dtype=np.uint64)
    return {"name": name, "circ": circ, "num_routed": R, "num_challenges": C, "log_n": LOG_N, "wires": wires,
            "cs": np.ascontiguousarray(np.concatenate([consts, sig.reshape(R, n)])), "pis": list(pis), "pih": pih, "gate": gate,
            "satisfied": tamper is None, "bad_rows": bad_rows, "accept": tamper is None and not over_degree}


# ---------------------------------------------------------------------------------------------------------------- the constraint kits
def _coefs_and_duplicates(o):
    """constant monomials (nf = 0), an empty constraint, duplicate monomials (another factor order, twice in one constraint, the same
    multiset in two constraints), coefficients that cancel (B = 0), and every int64 edge as a coefficient; outputs o, o + 1, ..."""
    return [
        ([(5, []), (3, [(W, 0), (W, 1)])], o),
        ([], None),                                                                   # n_mono = 0
        ([(7, [(W, 0), (W, 1)]), (11, [(W, 1), (W, 0)]), (1, [(W, 2), (W, 3)]), (1, [(W, 2), (W, 3)])], o + 1),
        ([(9, [(W, 4), (K, 1)]), (-9, [(K, 1), (W, 4)]), (2, [(W, 5)])], o + 2),
        ([(c, [(W, k), (W, k + 1)]) for k, c in enumerate(EDGE_COEFS)] + [(I64_MIN, []), (I64_MAX, [(K, 1)]), (I64_MIN, [(W, 3)])], o + 3),
    ]


def _power_runs(o, last_w, last_c, deg):
    """pure-power runs where the chained product must NOT fire (a gap w6, w6^3, w6^4; w3^2 then w4^3 on the next operand), runs where it
    must (constant 5: ^2, ^3), square-and-multiply up to `deg`, powers of selector columns and of pih words, the last wire and the last
    constant"""
    return [
        ([(1, [(W, 6)]), (2, [(W, 6)] * 3), (3, [(W, 6)] * 4)], o),
        ([(1, [(W, 3)] * 2), (-1, [(W, 4)] * 3), (5, [(W, 7)] * deg)], o + 1),
        ([(2, [(W, 5)]), (3, [(K, 5)] * 2), (4, [(K, 5)] * 3)], o + 2),
        ([(1, [(W, last_w)] * 2), (1, [(K, last_c)] * 3), (1, [(PIH, 3)] * 2), (1, [(PIH, 0), (W, last_w - 1)]), (1, [(K, 0)] * 2 + [(W, 8)]),
          (-1, [(PIH, 3)] * 3)], o + 3),
    ]


def single_selector(C=2, seed=1, tamper=None):
    """ONE selector column (many_sel = 0: no UNUSED - s factor): one group of four gates (filter degree 3) -- a no-op, constants and
    duplicates, pure-power runs, a gate whose constraints are all empty"""
    b = Builder()
    b.gate(0, 0, 0, 4, [])
    b.gate(0, 1, 0, 4, _coefs_and_duplicates(12))
    b.gate(0, 2, 0, 4, _power_runs(12, last_w=23, last_c=6, deg=MAX_DEGREE - 3))
    b.gate(0, 3, 0, 4, [([], None), ([], None)])
    circ = b.circuit(num_wires=24, num_routed=12, num_constants=7, num_selectors=1)
    return _witness(b, circ, seed, [1, 2, 3, 0, 2, 1], pis=[P - 1, 0, 1 << 32], cycles=40, tamper=tamper, C=C,
                    name="single_selector" if tamper is None else "single_selector_tampered")


def rich(C=3, seed=2, tamper=None):
    """three selector columns: a group of three gates (filter degree 3 with UNUSED), a ONE-gate group (filter UNUSED - s alone) holding
    the full chain w, w^2 .. w^7 and a separate w^7 by squaring, a group of two: wire 5 then constant 5 (^2, ^3) as ADJACENT pure powers
    once the compile step has sorted them (no wire above 5 in that gate), and a gate of empty constraints; operands at the last wire (not
    routed), the last constant and pih[3]"""
    b = Builder()
    b.gate(0, 0, 0, 3, _coefs_and_duplicates(14))
    b.gate(0, 1, 0, 3, _power_runs(14, last_w=29, last_c=5, deg=MAX_DEGREE - 3))
    b.gate(0, 2, 0, 3, [])
    b.gate(1, 3, 3, 4, [([(1 + k, [(W, 9)] * k) for k in range(1, 8)], 20), ([(1, [(W, 10)] * 7), (1, [(K, 4)] * 7)], 21),
                        ([(1, [(PIH, 1)] * 7), (-1, [(W, 11), (K, 1), (PIH, 2)])], 22)])
    b.gate(2, 4, 4, 6, [([(2, [(W, 5)]), (3, [(K, 5)] * 2), (4, [(K, 5)] * 3), (3, [(W, 0), (W, 29), (K, 5)]), (-2, [(K, 2), (K, 2), (PIH, 3)])], 4)])
    b.gate(2, 5, 4, 6, [([], None)])
    circ = b.circuit(num_wires=30, num_routed=16, num_constants=6, num_selectors=3)
    return _witness(b, circ, seed, [0, 1, 3, 4, 2, 5, 1, 3], pis=[1, 2, 3, 4, 5, 6, 7], cycles=50, tamper=tamper, C=C,
                    name="rich" if tamper is None else "rich_tampered")


def no_gate_constraints(C=4, seed=3):
    """every gate has zero constraints: num_gate_constraints = 0, only the permutation argument is in the quotient"""
    b = Builder()
    b.gate(0, 0, 0, 2, [])
    b.gate(0, 1, 0, 2, [])
    b.gate(1, 2, 2, 3, [])
    circ = b.circuit(num_wires=10, num_routed=9, num_constants=3, num_selectors=2)
    return _witness(b, circ, seed, [0, 1, 2], pis=[], cycles=20, C=C, name="no_gate_constraints")


def many_monomials(C=6, seed=4, n_mono=4096, last=(0, 0, 0)):
    """n_mono = 4096 in one constraint (the prover's limit; degree-2 monomials over 16 wires, so most merge), operands at the last index
    of each kind; `n_mono` / `last` (added to the last wire, constant, pih index) step over the limits"""
    Wn, Kn = 40, 4
    mono = [((k * 0x9E3779B1) % (1 << 40) - (1 << 39), [(W, k % 16), (W, (k // 16) % 16)]) for k in range(n_mono - 4)]
    mono += [(1, [(W, 37)]), (1, [(K, Kn - 1 + last[1])]), (1, [(PIH, 3 + last[2])])]
    b = Builder()
    b.gate(0, 0, 0, 1, [(mono, 38), ([(1, [(K, Kn - 1)] * 2)], 30)])
    b.gate(1, 1, 1, 2, [([(-1, [(W, 20), (W, 21)]), (1, [(W, Wn - 1 + last[0])])], 31)])
    circ = b.circuit(num_wires=Wn, num_routed=20, num_constants=Kn, num_selectors=2)
    if any(last) or n_mono != 4096:
        return circ                                                                   # outside the limits: the circuit alone
    return _witness(b, circ, seed, [0, 1, 0], pis=[9], cycles=10, C=C, name="many_monomials")


def pow64(C=7, seed=5, nf=64):
    """OVER-DEGREE: pure powers at the 64-factor limit (w^64 by squaring, w^63 then w^64 chained) and a mixed monomial of 64 factors
    over all three kinds, in a one-gate group; every row satisfies its programs, the quotient cannot hold them.  `nf` = 65 steps over"""
    b = Builder()
    mixed = [(W, 2)] * 30 + [(K, 2)] * 20 + [(PIH, 1)] * 10 + [(W, 3)] * (nf - 60)
    b.gate(0, 0, 0, 1, [([(1, [(W, 0)] * nf)], 10), ([(1, [(W, 1)] * 63), (1, [(W, 1)] * 64)], 11), ([(-1, mixed)], 12)])
    b.gate(1, 1, 1, 2, [([(1, [(W, 4), (W, 5)])], 13)])
    circ = b.circuit(num_wires=14, num_routed=8, num_constants=3, num_selectors=2)
    if nf != 64:
        return circ                                                                   # outside the limits: the circuit alone
    return _witness(b, circ, seed, [0, 1], pis=[3, 1, 4], C=C, name="pow64", over_degree=True)


def group64(C=2, seed=6, width=64):
    """OVER-DEGREE: one selector column, one group of 64 gates (filter degree 63); `width` = 65 steps over the prover's limit"""
    b = Builder()
    b.gate(0, 0, 0, width, [([(1, [(W, 0), (W, 1)])], 2)])
    for g in range(1, width - 1):
        b.gate(0, g, 0, width, [])
    b.gate(0, width - 1, 0, width, [([(2, [(W, 3)])], 4)])
    circ = b.circuit(num_wires=6, num_routed=4, num_constants=1, num_selectors=1)
    return _witness(b, circ, seed, [0, width - 1, 5, 0, 17], pis=[], C=C, name="group%d" % width, over_degree=True)


def big_counts(C=2, seed=7, num_wires=4096, num_constants=1024, num_constraints=4096):
    """the prover's count limits: 4096 wires, 1024 constants, 4096 constraints in one gate (most of them empty), operands at the last wire
    and constant; one more of any of them is refused by the prover alone (the oracle and both verifiers take it)"""
    b = Builder()
    cons = [([(1, [(W, 2 * k), (K, 2 + k)])], 2 * k + 1) for k in range(8)] + [([], None)] * (num_constraints - 9)
    b.gate(0, 0, 0, 1, cons + [([(1, [(W, num_wires - 2), (K, num_constants - 1)])], num_wires - 1)])
    b.gate(1, 1, 1, 2, [([(3, [(W, 0)])], 20)])
    circ = b.circuit(num_wires=num_wires, num_routed=8, num_constants=num_constants, num_selectors=2)
    return _witness(b, circ, seed, [0, 1, 1], pis=[5], cycles=8, C=C,
                    name="big_counts_%d_%d_%d" % (num_wires, num_constants, num_constraints))


# (id, entry function): the satisfied circuits (the richest at 1, 3 and 8 challenges), then the class every verifier refuses
ENTRIES = [("single_selector", single_selector), ("rich_C1", lambda: rich(C=1)), ("rich_C3", rich), ("rich_C8", lambda: rich(C=8)),
           ("no_gate_constraints", no_gate_constraints), ("many_monomials", many_monomials),
           ("pow64", pow64), ("group64", group64), ("single_selector_tampered", lambda: single_selector(tamper=(13, 4))),
           ("rich_tampered", lambda: rich(tamper=(20, 2)))]


def catalogue():
    return [f() for _, f in ENTRIES]


@functools.lru_cache(maxsize=None)
def limits():
    """the prover's own limits (circuit_check in sipp_amd/csrc/plonk.hip): (name, entry just inside, circuit just outside, the outside
    entry when the oracle's prover takes it, else None).  The oracle shares the nf / n_mono / operand limits, not the group width or the
    counts of wires, constants and constraints"""
    ins_mono, ins_nf, ins_w, ins_n = many_monomials(), pow64(), group64(), big_counts()
    wide = group64(width=65)
    out = [("group width", ins_w, wide["circ"], wide),
           ("nf", ins_nf, pow64(nf=65), None),
           ("n_mono", ins_mono, many_monomials(n_mono=4097), None)]
    for kind, name in ((0, "wire"), (1, "constant"), (2, "pih")):
        last = [0, 0, 0]
        last[kind] = 1
        out.append(("%s index" % name, ins_mono, many_monomials(last=tuple(last)), None))
    for key in ("num_wires", "num_constants", "num_constraints"):
        e = big_counts(**{key: (1025 if key == "num_constants" else 4097)})
        out.append((key, ins_n, e["circ"], e))
    return out


LIMIT_IDS = ["group width", "nf", "n_mono", "wire index", "constant index", "pih index", "num_wires", "num_constants", "num_constraints"]


# ---------------------------------------------------------------------------------------------------------------- reading a proof
def fri_params(entry):
    return _oracle.fri_params(rate_bits=FRI["rate_bits"], cap_height=FRI["cap_height"], pow_bits=6, num_queries=FRI["nq"], pow_rule=0, hiding=0,
                              arity_bits=FRI["arity"], final_poly_bits=FRI["fpb"], degree_bits=entry["log_n"])


def params(entry):
    return _oracle.plonk_params(entry["num_routed"], MAX_DEGREE, entry["num_challenges"])


_PROOFS = {}


def oracle_proof(entry):
    """orc_plonk_prove_gates of the entry under DIGEST, kept per (name, challenges): the catalogue is deterministic"""
    key = (entry["name"], entry["num_challenges"])
    if key not in _PROOFS:
        _PROOFS[key] = _oracle.plonk_prove_gates(entry["wires"], entry["cs"], entry["log_n"], params(entry), fri_params(entry), entry["circ"],
                                                 DIGEST, entry["pis"])
    return _PROOFS[key]


def sections(entry):
    """[(name, first word, end)] of a "SIPPPLK3" proof of this entry"""
    circ, R, C = entry["circ"], entry["num_routed"], entry["num_challenges"]
    cap = 4 << FRI["cap_height"]
    m = (R + MAX_DEGREE - 1) // MAX_DEGREE
    n_open = circ["num_constants"] + R + circ["num_wires"] + C * m + C * MAX_DEGREE + C
    head = 16 + 3 * cap
    return [("header", 0, 16), ("wires cap", 16, 16 + cap), ("Z cap", 16 + cap, 16 + 2 * cap), ("quotient cap", 16 + 2 * cap, head),
            ("openings", head, head + 8 + 2 * n_open), ("FRI", head + 8 + 2 * n_open, None)]


def first_difference(got, ref, entry):
    """None if the proofs are equal word for word, else where the first difference lies"""
    if len(got) != len(ref):
        return "length %d, the oracle's %d" % (len(got), len(ref))
    diff = np.flatnonzero(np.asarray(got) != np.asarray(ref))
    if diff.size == 0:
        return None
    k = int(diff[0])
    tail = len(ref) - len(entry["pis"])
    sec = "public inputs" if k >= tail else next(s for s, a, e in sections(entry) if a <= k and (e is None or k < e))
    return "%s: first differing word %d of %d (%s), %d words differ" % (entry["name"], k, len(ref), sec, diff.size)
