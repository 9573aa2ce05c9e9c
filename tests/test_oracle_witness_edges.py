"""The witness generators' edge catalogue (tests/_witness_edges.py) on the CPU: its exact Python-integer reference against
oracle/plonk_witness.c (kinds 1 .. 8) and tests/_merkle_reading.py (the swap rows and the mixed lists), on every launch plan of every
entry; the gate constraints of tools/plonk_synth.circuit_recursion_shaped and of sipp_amd.merkle.poseidon_swap_gate vanish on the expected
rows that use their layouts; the coverage the catalogue promises (every crafted row carries in its output of the first MDS layer, the
p - 1 product, an index beyond every random-access table, every arithmetic tuple) holds, computed from the reference alone."""
import itertools
import os
import sys

import numpy as np
import pytest

from sipp_amd import merkle as mk
from tests import _merkle_reading as mr
from tests import _oracle
from tests import _witness_edges as we
from tests import _witness_reading as rd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plonk_synth as ps  # noqa: E402

P = we.P
NAMES = [name for name, _ in we.ENTRIES]
POSEIDON_NAMES = [n for n in NAMES if n.startswith("poseidon")]


def held(e, g):
    """does any row hold the generator's selector value?"""
    return bool((e["consts"][g[1]] == np.uint64(g[2])).any())


def c_reading(e, gens, sched):
    """oracle/plonk_witness.c; a swap generator (which it does not know) only where no row holds it"""
    assert not any(g[0] == we.POSEIDON_SWAP and held(e, g) for g in gens)
    gens = [g for g in gens if g[0] != we.POSEIDON_SWAP]
    if sched is None:
        return _oracle.plonk_generate_witness(e["wires"], e["consts"], e["log_n"], gens, e["pih"])
    return _oracle.plonk_generate_witness_levels(e["wires"], e["consts"], e["log_n"], gens, e["pih"], sched)


def merkle_reading(e, gens, sched):
    if sched is None:
        return rd.row_local(e["wires"], e["consts"], gens, e["pih"])
    return rd.replay(e["wires"], e["consts"], gens, e["pih"], sched)


@pytest.mark.parametrize("name,path", we.cases(), ids=["%s-%s" % c for c in we.cases()])
def test_reference_equals_the_other_readings_on_every_plan(name, path):
    """the expected table = the reference on the plan's own generator list and schedule = oracle/plonk_witness.c (lists without a held
    swap generator) = tests/_merkle_reading.py (lists of the families it reads); boundary_swap, which neither reads whole, row by row:
    the C reading on the rows of kinds 1 .. 8, the Merkle reading's swap generator on the swap rows (no copies: the rows are independent)"""
    e = we.entry(name)
    gens, sched = we.plan(e, path)
    again, written = we.generate(e["wires"], e["consts"], gens, e["pih"], sched)
    assert we.first_mismatch(e, again) is None and (written == e["written"]).all()
    has_swap = any(g[0] == we.POSEIDON_SWAP and held(e, g) for g in gens)
    merkle_kinds = {rd.GEN_CONSTANT, rd.GEN_PUBLIC_INPUT, rd.GEN_BASE_SPLIT, rd.GEN_RANDOM_ACCESS, rd.GEN_POSEIDON, rd.GEN_POSEIDON_SWAP}
    if not has_swap:
        assert we.first_mismatch(e, c_reading(e, gens, sched)) is None
    if all(g[0] in merkle_kinds or not held(e, g) for g in gens):
        assert we.first_mismatch(e, merkle_reading(e, [g for g in gens if g[0] in merkle_kinds], sched)) is None
    elif has_swap:
        assert name == "boundary_swap" and not len(sched["copy_src"])
        swap_row = e["kind"] == we.POSEIDON_SWAP
        scheduled = np.zeros(1 << e["log_n"], dtype=bool)
        scheduled[sched["rows"]] = True
        c = _oracle.plonk_generate_witness_levels(e["wires"], e["consts"], e["log_n"], [g for g in gens if g[0] != we.POSEIDON_SWAP], e["pih"], sched)
        m = rd.replay(e["wires"], e["consts"], [g for g in gens if g[0] == we.POSEIDON_SWAP], e["pih"], sched)
        assert (c[:, ~swap_row] == e["expected"][:, ~swap_row]).all() and (m[:, swap_row] == e["expected"][:, swap_row]).all()
        assert (swap_row & scheduled).sum() > 1000 and (m[:, ~swap_row] == e["wires"][:, ~swap_row]).all()


@pytest.mark.parametrize("name", NAMES)
def test_entries_are_what_the_catalogue_says(name):
    """generated cells hold the sentinel before and no longer after (but where the generated value IS an input copied through), cells
    outside `written` are unchanged, every plan runs the kernels its path names, at most 16 generators"""
    e = we.entry(name)
    n = 1 << e["log_n"]
    assert e["wires"].shape == (e["num_wires"], n) and e["consts"].shape == (e["num_constants"], n)
    assert (e["wires"][e["written"]] == we.SENTINEL).all()
    assert (e["expected"][~e["written"]] == e["wires"][~e["written"]]).all()
    assert e["written"].any() and not e["written"][:, e["consts"][0] == we.OTHER].any()
    assert (e["consts"][0] == we.OTHER).sum() >= 1
    for path in e["paths"]:
        gens, sched = we.plan(e, path)
        assert len(gens) <= 16
        if sched is not None:
            ks = we.kernels(gens, sched)
            assert ks == ({path, "wide"} if name.startswith("boundary") else {path}), (name, path, ks)
            assert len(set(sched["rows"].tolist())) == len(sched["rows"]) and len(set(sched["copy_dst"].tolist())) == len(sched["copy_dst"])
    assert tuple(p for nm, p in we.cases() if nm == name) == e["paths"]


def test_every_crafted_row_carries_in_its_output_and_every_output_is_covered():
    """from the reference state alone: al, ah and lo < al of the first MDS layer.  Over the Poseidon entries every output 0 .. 11 carries,
    with the solved element on the diagonal (for output 0: the coefficient that holds the diagonal term's 8) and off it; uniform states
    do not carry (the reason for the crafted ones)"""
    for diagonal in (True, False):
        for r in range(12):
            assert we.first_layer_carries(we.crafted_state(r, diagonal))[r]
    rng = np.random.default_rng(1)
    assert not any(any(we.first_layer_carries([int(x) for x in _oracle.rand_field(rng, 12)])) for _ in range(2000))
    assert not any(we.first_layer_carries([P - 1] * 12)) and not any(we.first_layer_carries([0] * 12))
    for name in POSEIDON_NAMES + ["thin_levels_plain", "thin_levels_swap", "boundary_plain", "boundary_swap"]:
        e = we.entry(name)
        assert e["crafted"], name
        seen = {}
        for row, r in e["crafted"]:
            key = tuple(we.state_of(e, row))
            if key not in seen:
                seen[key] = we.first_layer_carries(list(key))
            assert seen[key][r], (name, row, r)
            assert e["kind"][row] in (we.POSEIDON, we.POSEIDON_SWAP)
        if not name.startswith("thin"):
            assert {r for _, r in e["crafted"]} == set(range(12)), name
            assert len(seen) >= 24                                     # diagonal and off-diagonal, per output


def test_no_poseidon_or_arithmetic_case_is_left_out():
    states = we.poseidon_states()
    assert len(states) == 2 + 9 + 12 + 1 + 24
    for which in ("upstream", "shifted", "last"):
        e = we.entry("poseidon_%s" % which)
        got = {tuple(we.state_of(e, r)) for r in np.flatnonzero(e["kind"] == we.POSEIDON)}
        assert got == {tuple(st) for _, st, _ in states}
        e = we.entry("poseidon_swap_%s" % which)
        rows = np.flatnonzero(e["kind"] == we.POSEIDON_SWAP)
        sw = e["gens"][0][6]
        for s in (0, 1, 2, P - 1):                                     # every plain state under every swap value
            ins = {tuple(int(e["wires"][e["gens"][0][3] + i, r]) for i in range(12)) for r in rows if int(e["wires"][sw, r]) == s}
            assert {tuple(st) for _, st, c in states if c is None} <= ins
        for s in (0, 1):                                               # the permutation runs on every crafted state under swap 0 and 1
            run = {tuple(we.state_of(e, r)) for r in rows if int(e["wires"][sw, r]) == s}
            assert {tuple(st) for _, st, c in states if c is not None} <= run
        i0 = e["gens"][0][3]
        assert any(int(e["wires"][i0, r]) == P - 1 and int(e["wires"][i0 + 4, r]) == 0 for r in rows)              # 0 - (p - 1)
    tuples = set(itertools.product(we.EDGE, repeat=5))
    assert len(tuples) == 7776
    for n_ops in (1, 34):
        e = we.entry("arithmetic_%d" % n_ops)
        rows = np.flatnonzero(e["kind"] == we.ARITHMETIC)
        for op in {0, n_ops - 1}:
            got = {(int(e["consts"][we.C0, r]), int(e["consts"][we.C1, r])) + tuple(int(e["wires"][4 * op + j, r]) for j in range(3)) for r in rows}
            assert got == tuples, (n_ops, op)
    assert e["written"][135].any()                                      # 34 ops: the last wire is written
    b = we.entry("boundary_plain")
    rows = np.flatnonzero(b["kind"][:16383] == we.ARITHMETIC)
    assert {(int(b["consts"][we.C0, r]), int(b["consts"][we.C1, r])) + tuple(int(b["wires"][j, r]) for j in range(3)) for r in rows} == tuples


def test_short_families_hold_their_named_edges():
    e = we.entry("u32_mul_add")
    assert we.U32_P_MINUS_1 in we.U32_TRIPLES and (we.M32 * we.M32 + we.M32) == P - 1
    for g in e["gens"]:                                                 # the p - 1 result in op 0 of every layout: low half 0, high half 0xFFFFFFFF
        rows = np.flatnonzero(e["consts"][0] == np.uint64(g[2]))
        hit = [r for r in rows if tuple(int(e["wires"][j, r]) for j in range(3)) == we.U32_P_MINUS_1]
        assert hit and all(int(e["expected"][3, r]) == 0 and int(e["expected"][4, r]) == we.M32 for r in hit)
        assert any(int(e["wires"][0, r]) > we.M32 for r in rows)        # an operand that is no u32
    wide = next(g for g in e["gens"] if g[3:6] == (3, 45, 16))          # the gap cells of the wide stride are no generator's
    assert not e["written"][37:45].any() or not e["written"][37:45, e["consts"][0] == np.uint64(wide[2])].any()
    assert e["written"][135].any()
    e = we.entry("random_access")
    for g in e["gens"]:
        rows = np.flatnonzero(e["consts"][0] == np.uint64(g[2]))
        assert any(int(e["wires"][0, r]) >= 1 << g[5] for r in rows) and any(int(e["wires"][0, r]) == (1 << g[5]) - 1 for r in rows)
    assert {g[5] for g in e["gens"]} == {1, 2, 6} and e["written"][135].any()
    e = we.entry("base_split")
    assert {(g[3], g[4]) for g in e["gens"]} >= {(1, 1), (1, 32), (2, 32), (64, 1), (63, 1), (32, 2), (16, 4), (21, 3)}
    for g in e["gens"]:
        vals = {int(e["wires"][0, r]) for r in np.flatnonzero(e["consts"][0] == np.uint64(g[2]))}
        top = g[3] * g[4]
        assert set(we.MORE) <= vals and (top == 64 or any(v >> top for v in vals))
        for k in range(g[4], top + 1, g[4]):                            # both sides of every limb boundary (2^64 - 1 and 2^64 are no field elements)
            assert all(v in vals or v >= P for v in ((1 << k) - 1, 1 << k)), (g, k)
    e = we.entry("reducing")
    assert {(g[3], g[4]) for g in e["gens"]} >= {(44, 7), (44, 0), (44, 1), (44, we.M32), (1, 7)} and e["written"][135].any()
    e = we.entry("constant_public_input_a")
    assert {g[3] for g in e["gens"] if g[0] == we.CONSTANT} >= {0, 1, we.NUM_CONSTANTS - 1}


def test_both_sides_of_the_kernel_switch_hold_the_same_rows_and_expect_the_same():
    for name in ("boundary_plain", "boundary_swap"):
        e = we.entry(name)
        lo = e["sched"]["level_offsets"]
        assert list(np.diff(lo.astype(np.int64))) == [16383, 16384]
        a, b = e["sched"]["rows"][:16383].astype(np.int64), e["sched"]["rows"][16383:16383 + 16383].astype(np.int64)
        assert (b == a + 16384).all()
        assert (e["wires"][:, a] == e["wires"][:, b]).all() and (e["consts"][:, a] == e["consts"][:, b]).all()
        assert (e["expected"][:, a] == e["expected"][:, b]).all()
        assert (e["expected"][:, 16383] == e["wires"][:, 16383]).all() and e["written"][:, 32767].any()
        kinds = e["kind"][:16384].reshape(-1, 4)                         # blocks of four rows: Poseidon only, short only, mixed
        is_p = (kinds == we.POSEIDON) | (kinds == we.POSEIDON_SWAP)
        assert is_p.all(axis=1).any() and (~is_p).all(axis=1).any() and (is_p.any(axis=1) & ~is_p.all(axis=1)).any()


def test_thin_levels_have_the_sizes_and_the_copies():
    for name in ("thin_levels_plain", "thin_levels_swap"):
        e = we.entry(name)
        sizes = list(np.diff(e["sched"]["level_offsets"].astype(np.int64)))
        assert set(sizes) == {1, 2, 3, 5} and len(e["sched"]["copy_src"]) >= 8
        n = 1 << e["log_n"]
        row0 = int(e["sched"]["rows"][0])                                # level 0: ONE crafted Poseidon row; its outputs feed a later level
        assert (row0, ) == tuple(r for r, _ in e["crafted"][:1]) and sizes[0] == 1
        first = e["sched"]["copy_src"][:int(e["sched"]["copy_offsets"][1])]
        assert len(first) and (first % np.uint64(n) == np.uint64(row0)).all()
        dst = e["sched"]["copy_dst"].astype(np.int64)
        assert (e["wires"].reshape(-1)[dst] == we.SENTINEL).all()
        assert (e["expected"].reshape(-1)[dst] == e["expected"].reshape(-1)[e["sched"]["copy_src"].astype(np.int64)]).all()
        assert (e["expected"].reshape(-1)[dst] != we.SENTINEL).all()


# ---- the gate constraints on the expected rows ---------------------------------------------------------------------------------------
RECURSION_GATES = {(we.BASE_SPLIT, 32, 1): (0, 2), (we.PUBLIC_INPUT,): (0, 3), (we.CONSTANT, 2, 3): (0, 4), (we.U32_MUL_ADD, 3, 37, 16): (1, 5),
                   (we.RANDOM_ACCESS, 10, 8, 2): (1, 6), (we.REDUCING, 40, 7): (1, 7), (we.POSEIDON, 0, 12, 24): (2, 8)}


def _in_range(e, g, r):
    """does the row hold what the gate's constraints allow (u32 operands, an index inside the table, a value of 32 bits)?"""
    w = lambda j: int(e["wires"][j, r])
    if g[0] == we.U32_MUL_ADD:
        return all(w(g[4] * op + j) <= we.M32 for op in range(g[3]) for j in range(3))
    if g[0] == we.RANDOM_ACCESS:
        return all(w(g[4] * cp) < 1 << g[5] for cp in range(g[3]))
    if g[0] == we.BASE_SPLIT:
        return w(0) < 1 << (g[3] * g[4])
    return True


@pytest.mark.parametrize("name", ["base_split", "constant_public_input_a", "constant_public_input_b", "u32_mul_add", "random_access", "reducing",
                                  "poseidon_upstream"])
def test_recursion_shaped_constraints_vanish_on_the_expected_rows(name):
    """the generators whose layout is tools/plonk_synth.circuit_recursion_shaped's: every constraint of the row's gate vanishes on the
    expected row (oracle/plonk_gates.c on every row, tools/plonk_synth.check_rows on a sample), where the inputs are in the gate's range;
    where they are not (an operand beyond u32, an index beyond the table, a value beyond the limbs) some constraint does not"""
    e = we.entry(name)
    circ = ps.circuit_recursion_shaped(136, 80)
    checked = 0
    for g in e["gens"]:
        key = (g[0],) + tuple(g[3:3 + {we.PUBLIC_INPUT: 0, we.BASE_SPLIT: 2, we.CONSTANT: 2, we.REDUCING: 2}.get(g[0], 3)])
        if key not in RECURSION_GATES:
            continue
        si, gate = RECURSION_GATES[key]
        rows = np.flatnonzero(e["consts"][g[1]] == np.uint64(g[2]))
        cs = np.full((5, len(rows)), ps.UNUSED, dtype=np.uint64)
        cs[si] = gate
        cs[3:5] = e["consts"][3:5, rows]
        w = np.ascontiguousarray(e["expected"][:136, rows])
        ok = [_in_range(e, g, r) for r in rows]
        for k in range(len(rows)):
            zero = not _oracle.plonk_gate_constraints_base(circ, np.ascontiguousarray(w[:, k]), np.ascontiguousarray(cs[:, k]), e["pih"]).any()
            assert zero == ok[k], (name, we.FAMILY[g[0]], int(rows[k]))
        sample = [k for k in range(len(rows)) if ok[k]][::max(1, len(rows) // 12)]
        assert sample and ps.check_rows(circ, w, cs, e["pih"], sample)
        checked += len(rows)
    assert checked


def _eval_exact(cons, col):
    out = []
    for monos in cons:
        s = 0
        for coef, fs in monos:
            t = coef
            for kind, idx in fs:
                assert kind == 0
                t = t * col[idx] % P
            s = (s + t) % P
        out.append(s)
    return out


@pytest.mark.parametrize("which", ["upstream", "shifted", "last"])
def test_swap_gate_constraints_vanish_on_the_expected_rows(which):
    """sipp_amd.merkle.poseidon_swap_gate in the entry's layout: all 123 constraints vanish on every expected row with swap 0 or 1; with
    swap 2 or p - 1 booleanity alone does not (oracle/plonk_gates.c on every row; the decoded program over Python integers on a sample,
    the crafted rows among it)"""
    e = we.entry("poseidon_swap_%s" % which)
    nw, lay = we.SWAP_LAYOUTS[which]
    prog = mk.poseidon_swap_gate(**lay)
    circ = {"num_wires": nw, "num_routed": 80, "num_constants": 1, "num_selectors": 1, "gates": [(0, 0, 0, 1, 0, 123)], "programs": prog,
            "num_gate_constraints": 123}
    cons = mr.decode(prog, 0, 123)
    rows = np.flatnonzero(e["kind"] == we.POSEIDON_SWAP)
    crafted = {r for r, _ in e["crafted"]}
    for k, r in enumerate(rows):
        col = np.ascontiguousarray(e["expected"][:, r])
        bad = set(np.flatnonzero(_oracle.plonk_gate_constraints_base(circ, col, np.zeros(1, dtype=np.uint64), [0, 0, 0, 0])).tolist())
        want = set() if int(e["wires"][lay["swap"], r]) in (0, 1) else {0}
        assert bad == want, (which, int(r), bad)
        if k % 40 == 0 or (r in crafted and k % 12 == 0):
            assert {j for j, v in enumerate(_eval_exact(cons, [int(x) for x in col])) if v} == want, (which, int(r))
