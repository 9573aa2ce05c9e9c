"""SIPP's transcript in the outer circuit on the CPU (sipp_amd/nonnative.py, sipp_amd/transcript.py): the catalogue of
tests/_transcript_cases.py reaches the generators' edges; for n = 4 and n = 8 the witness replayed by the Python reading satisfies every
row and every cycle, its x / x^-1 cells are the fixtures' exponents, the oracle proves and both verifiers accept; forged quotients,
remainders, inverses, limbs and carries fail where the soundness argument says; tampered inputs are refused by both verifiers; the
circuits' shapes are the pinned ones (tests/golden/transcript_circuit_shapes.json, tools/transcript_circuit_shapes.py)."""
import json
import os
import sys

import numpy as np
import pytest

from sipp_amd import nonnative as nn
from sipp_amd import transcript as tr
from tests import _oracle, _verify
from tests import _transcript_cases as tc
from tests import _witness_reading as rd
from tests.test_oracle_plonk import fri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "transcript_circuit_shapes.json")
P, R, M32 = tc.P, tc.R, tc.M32
DIGEST = (61, 62, 63, 64)
SIZES = (4, 8)
_built = {}


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
def test_the_catalogue_reaches_its_edges():
    C = tc.CATALOGUE
    reduce_r = [a for k, (kind, a) in C.items() if kind == "reduce" and a[1] == R]
    assert {x // R for x, _ in reduce_r} == {0, 1, 2, 3, 4, 5} and (1 << 256) // R == 5
    assert {x for x, _ in reduce_r} >= {0, 1, R - 1, R, R + 1, 5 * R - 1, 5 * R, (1 << 256) - 1}
    assert any(set(tc.limbs(x)) == {0, M32} for x, _ in reduce_r)
    assert {a[1] for k, (kind, a) in C.items() if kind == "reduce"} >= {R, tc.Q, 3}
    inv_r = {a[0] for kind, a in C.values() if kind == "inverse" and a[1] == R}
    assert inv_r >= {1, 2, R - 1, R + 1} and any(x >> 255 for x in inv_r)
    assert any(kind == "inverse" and a[1] == 3 for kind, a in C.values())
    # every refusal shape, and the reading refuses exactly those
    refused = {k: C[k][1] for k in tc.REFUSED}
    assert refused["reduce_refused_m_0"][1] == 0 and refused["inverse_refused_m_0"][1] == 0
    assert refused["inverse_refused_m_even"][1] % 2 == 0 and refused["inverse_refused_m_1"][1] == 1
    assert refused["inverse_refused_x_0"][0] == 0 and refused["inverse_refused_gcd"] == (5, 15)
    for k, (kind, a) in C.items():
        if kind in ("reduce", "inverse"):
            assert (tc.nonnative(kind == "inverse", *a) is None) == (k in tc.REFUSED), k
    # u32 arithmetic: the value p - 1 (hi all ones, lo 0, inverse cell 0), zero, 2^32 - 2, exactly 2^32, operands with bits above 32
    w = [M32, M32, M32] + [7] * 40
    tc.u32_arithmetic_row(w, 1, 38, 16)
    assert w[3:6] == [0, M32, 0] and w[3] + (w[4] << 32) == P - 1 and w[6:22] == [0] * 16 and w[22:38] == [3] * 16
    values = {(a & M32) * (b & M32) + (c & M32) for kind, arg in C.values() if kind == "arith" for a, b, c in [arg]}
    assert values >= {P - 1, 0, (1 << 32) - 2, 1 << 32}
    assert any(max(arg) >> 32 for kind, arg in C.values() if kind in ("arith", "add"))
    # add-many: both carry extremes (0 and 16: sixteen addends and the carry-in at their maxima), a single addend, zero
    carries = {sum(v & M32 for v in arg) >> 32 for kind, arg in C.values() if kind == "add"}
    assert carries >= {0, 16} and max(carries) == 16 == (17 * M32) >> 32
    assert any(kind == "add" and sum(1 for v in arg if v) == 1 and arg[0] for kind, arg in C.values())
    # the table: every case on a row, the refused rows all zero in their 24 cells, every other written cell as the reading says
    wires, k, gens, want, names = tc.catalogue_table(6, repeat=False)
    assert names == sorted(C) and len(names) <= 64
    for r, name in enumerate(names):
        kind, a = C[name]
        if kind in ("reduce", "inverse"):
            got = tc.nonnative(kind == "inverse", *a)
            cells = [int(v) for v in want[16:40, r]]
            assert cells == ([0] * 24 if got is None else tc.limbs(got[0]) + tc.limbs(got[1]) + tc.limbs(got[2])), name
            if got is not None:
                x, m = a
                assert (x == got[1] * m + got[0] if kind == "reduce" else x * got[0] == got[1] * m + 1) and got[0] + got[2] + 1 == m
    assert (want[:, len(names):] == wires[:, len(names):]).all()


def test_the_gate_programs_hold_on_every_catalogue_row_of_their_gate():
    """the u32 gates as one-gate circuits over the catalogue's rows (the reading's values)"""
    wires, k, gens, want, names = tc.catalogue_table(6, repeat=False)
    for sel, fill, args in ((1, nn.u32_arithmetic_into, (2, 38, 16)), (2, nn.u32_add_many_into, (1, 38, 16, 3))):
        circ = one_gate(fill, *args)
        rows = np.flatnonzero(k[0] == sel)
        assert len(rows) >= 5
        for r in rows:
            # operands that are not u32 are the constraints' to refuse: the generator's low-32-bit reading does not satisfy the gate
            assert bool(nonzero(circ, want[:, r])) == ("bits_above_32" in names[r]), names[r]


def one_gate(fill, *args):
    from sipp_amd.circuit import _words
    pr, words = _words(fill, *args)
    return {"num_wires": tc.NUM_WIRES, "num_routed": 80, "num_constants": 1, "num_selectors": 1, "gates": [(0, 0, 0, 1, 0, pr.count)],
            "programs": words, "num_gate_constraints": pr.count}


def nonzero(circ, row):
    return set(np.flatnonzero(_oracle.plonk_gate_constraints_base(circ, np.ascontiguousarray(row), np.zeros(1, dtype=np.uint64), [0, 0, 0, 0])).tolist())


def test_the_other_split_of_a_small_value_fails_the_canonicity_constraint_alone():
    """V = 2^32 - 2 = 1 (2^32 - 2) + 0: V + p = 2^64 - 1 is (lo, hi) = (2^32 - 1, 2^32 - 1), which meets the product constraint mod p
    and every limb constraint; only (inverse (2^32 - 1 - hi) - 1) lo = 0 refuses it, whatever the inverse cell holds"""
    circ = one_gate(nn.u32_arithmetic_into, 1, 38, 16)
    for V, (a, b, c) in ((M32 - 1, (1, M32 - 1, 0)), (0, (0, 5, 0)), (77, (7, 11, 0))):
        w = [a, b, c] + [0] * (tc.NUM_WIRES - 3)
        tc.u32_arithmetic_row(w, 1, 38, 16)
        assert w[3] + (w[4] << 32) == V and not nonzero(circ, np.array(w, dtype=np.uint64))
        other = V + P
        assert other < 1 << 64
        lo, hi = other & M32, other >> 32
        assert hi == M32 and lo == V + 1
        for inv in (0, 1, w[5], P - 1):
            f = list(w)
            f[3:6] = [lo, hi, inv]
            f[6:22] = [(lo >> (2 * l)) & 3 for l in range(16)]
            f[22:38] = [3] * 16
            assert nonzero(circ, np.array(f, dtype=np.uint64)) == {1}, (V, inv)


# ---- the circuit ------------------------------------------------------------------------------------------------------------------------
def build(n):
    if n not in _built:
        c = tr.SippTranscriptCircuit(n)
        st, rw, ex, d = tc.fixture(n)
        cs = c.constants_sigmas()
        _built[n] = {"c": c, "st": st, "rw": rw, "ex": ex, "npz": d, "cs": cs, "ch": tr.challenges_of(d["fq12"]),
                     "cs_cap": _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap}
    return _built[n]


def witness(b, st=None, rw=None, ch=None):
    c = b["c"]
    args = (b["st"] if st is None else st, b["rw"] if rw is None else rw, b["ch"] if ch is None else ch)
    pis = c.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    return rd.replay(c.partial_witness(*args), b["cs"][:c.num_constants], c.generators(), pih, c.schedule()), pis, pih


def honest(n):
    b = build(n)
    if "w" not in b:
        b["w"], b["pis"], b["pih"] = witness(b)
    return b


def bad_rows(b, w, pih):
    c, circ = b["c"], b["c"].circuit()
    return [r for r in range(c.n) if _oracle.plonk_gate_constraints_base(circ, w[:, r], b["cs"][:c.num_constants, r], pih).any()]


def bad_cycles(b, w):
    flat = w.reshape(-1)
    return [cyc for cyc in b["c"].cycles if len(set(flat[np.asarray(cyc, dtype=np.int64)].tolist())) != 1]


def prove_and_judge(b, w, pis):
    c = b["c"]
    op = _oracle.plonk_params(80, 8, 2)
    ofp = fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    circ = c.circuit()
    pf = _oracle.plonk_prove_gates(w, b["cs"], c.log_n, op, ofp, circ, DIGEST, pis)
    return _oracle.plonk_verify_gates(pf, b["cs_cap"], op, ofp, circ, DIGEST), _verify.lib_plonk_verify(pf, b["cs_cap"], op, ofp, circ, DIGEST)


def cell_value(w, cells):
    return tc.value([int(w[wire, row]) for wire, row in cells])


@pytest.mark.parametrize("n", SIZES)
def test_the_replayed_witness_satisfies_every_row_and_cycle_and_holds_the_fixtures_exponents(n):
    b = honest(n)
    c, w = b["c"], b["w"]
    assert bad_rows(b, w, b["pih"]) == [] and bad_cycles(b, w) == []
    out, digests, perms = tc.transcript(_oracle.hash_no_pad, b["st"], b["rw"])
    assert len(c.transcript_rows) == perms == {4: 99, 8: 158}[n]
    assert out == b["ex"]                                       # the eight-limb reading reproduces the recorded exponents
    assert all(d >> 32 and d < P for dg in digests for d in dg)   # no digest word with a zero high half: the native reading agrees
    for k in range(c.rounds):
        x, xi = cell_value(w, c.x_cells[k]), cell_value(w, c.xinv_cells[k])
        assert (x, xi) == b["ex"][k] and x * xi % R == 1 and x < R and xi < R
        assert cell_value(w, c.digest_limbs[k]) == sum(d << (64 * i) for i, d in enumerate(digests[k]))
    # the generated cells equal exp_val in every g1, g2 and fq12 record
    d, at = b["npz"], 0
    for k in range(c.rounds):
        x, xi = tc.limbs(b["ex"][k][0]), tc.limbs(b["ex"][k][1])
        for _ in range(n >> (k + 1)):
            assert [int(v) for v in d["g1"][at, 32:40]] == x and [int(v) for v in d["g2"][at, 64:72]] == xi
            at += 1
        assert [int(v) for v in d["fq12"][2 * k, 192:200]] == x and [int(v) for v in d["fq12"][2 * k + 1, 192:200]] == xi
    assert at == len(d["g1"]) == len(d["g2"]) == n - 1
    assert b["pis"][c.n_statement:] == b["ch"] and (w[12:16, c.chain_row[-1]] == np.array(b["pih"], dtype=np.uint64)).all()


@pytest.mark.parametrize("n", SIZES)
def test_the_oracle_proves_and_both_verifiers_accept(n):
    b = honest(n)
    assert prove_and_judge(b, b["w"], b["pis"]) == (0, 0)


def test_the_circuit_shape():
    c = build(4)["c"]
    circ = c.circuit()
    degrees = {"Noop": 0, "PublicInput": 1, "Constant": 1, "BaseSplit64": 2, "LeSum32": 2, "NonnativeInverse": 0, "U32Range": 4,
               "U32Arithmetic": 4, "U32AddMany": 4, "NonnativeReduce": 0, "PoseidonSwap": 7}
    from tests import _merkle_reading as mr
    for (si, row, lo, hi, off, nc), name in zip(circ["gates"], circ["gate_names"]):
        cons = mr.decode(circ["programs"], off, nc)
        assert max([len(f) for cn in cons for _, f in cn] or [0]) == degrees[name], name
        assert (hi - lo - 1) + 1 + degrees[name] <= 8
    assert [g[5] for g in circ["gates"]] == [0, 4, 1, 65, 33, 0, 17, 72, 22, 0, 123]
    assert c.n_pi == 48 * 4 + 96 + 32 and len(c.in_cycle) == 2 * 192
    per_round = {"range": 48, "arith": 3 * 32, "add": 3 * 16 + 2 * 8, "reduce": 1, "inverse": 1}
    assert {k: len(v) for k, v in c.u32_rows.items()} == {k: 2 * v for k, v in per_round.items()}
    assert len(c.generators()) == 10 and max(max(cyc) for cyc in c.cycles) < 80 * c.n


# ---- forgeries ----------------------------------------------------------------------------------------------------------------------------
class forged_nonnative:
    """the reading of kind 21 with the outputs of one row replaced: forge(result, quotient, x, m) -> (result, quotient); the slack is
    the forger's best, m - 1 - result mod 2^256"""

    def __init__(self, row, forge):
        self.row, self.forge = row, forge

    def __enter__(self):
        self.saved = rd.READINGS[tc.GEN_NONNATIVE]

        def on_rows(wires, consts, pih, p, rows):
            self.saved(wires, consts, pih, p, rows)
            if self.row in [int(r) for r in rows]:
                col = [int(v) for v in wires[:, self.row]]
                x, m = tc.value(col[0:8]), tc.value(col[8:16])
                res, quo = self.forge(tc.value(col[16:24]), tc.value(col[24:32]), x, m)
                wires[16:40, self.row] = np.array(tc.limbs(res) + tc.limbs(quo) + tc.limbs((m - 1 - res) % (1 << 256)), dtype=np.uint64)
        rd.READINGS[tc.GEN_NONNATIVE] = on_rows

    def __exit__(self, *exc):
        rd.READINGS[tc.GEN_NONNATIVE] = self.saved


def less_than_top(b, k, inverse):
    """(the cycle of, the row of) the top carry of round k's result + slack + 1 = m chain.  The builder makes a round's add-many rows in
    order: reduce's sixteen columns and eight less-than limbs, then inverse's two products and eight less-than limbs -- 64 a round"""
    c = b["c"]
    top = c.u32_rows["add"][64 * k + (63 if inverse else 23)]
    return next(cyc for cyc in c.cycles if (nn.ADD_ADDENDS + 2) * c.n + top in cyc), top


@pytest.mark.parametrize("what", ["rem_plus_r_with_q_minus_1", "inv_plus_r"])
def test_a_congruent_but_larger_remainder_or_inverse_breaks_the_less_than_carry(what):
    """n = 4.  The forger writes rem + r beside q - 1 (on a round where q >= 1), or inv + r beside k + x: x = q m + rem and x inv = k m
    + 1 still hold limb for limb, every limb is a u32 and every gate constraint holds; the forger even claims the forged limbs as the
    public challenge.  What fails is the top carry of result + slack + 1 = m, tied to zero: the result is not below m."""
    b = honest(4)
    c, w0 = b["c"], b["w"]
    if what == "rem_plus_r_with_q_minus_1":
        k = next(k for k in range(c.rounds) if cell_value(w0, [(24 + t, c.u32_rows["reduce"][k]) for t in range(8)]) >= 1)
        row, forge = c.u32_rows["reduce"][k], lambda res, quo, x, m: (res + m, quo - 1)
    else:
        k = 0
        row, forge = c.u32_rows["inverse"][k], lambda res, quo, x, m: (res + m, quo + x)
    # the forger claims the forged limbs as the public challenge (the other value of the round is what it was: rem + r has rem's inverse)
    ch = list(b["ch"])
    at = 16 * k + (8 if what == "inv_plus_r" else 0)
    ch[at:at + 8] = tc.limbs(tc.value(ch[at:at + 8]) + R)
    with forged_nonnative(row, forge):
        w, pis, pih = witness(b, ch=ch)
    assert cell_value(w, [(16 + t, row) for t in range(8)]) == cell_value(w0, [(16 + t, row) for t in range(8)]) + R
    assert bad_rows(b, w, pih) == []
    cyc, top = less_than_top(b, k, what == "inv_plus_r")
    assert int(w[nn.ADD_ADDENDS + 2, top]) == 1
    assert bad_cycles(b, w) == [cyc]
    if what == "inv_plus_r":
        assert prove_and_judge(b, w, pis) == (-210, 210)


def test_a_limb_of_4_and_a_nonzero_top_carry_fail_on_their_rows():
    b = honest(4)
    c = b["c"]
    # a two-bit cell holding 4, the limb above lowered so that the sum still is the value
    r = next(r for r in c.u32_rows["range"] if int(b["w"][2, r]) >= 1)
    w = b["w"].copy()
    w[1, r] += np.uint64(4)
    w[2, r] -= np.uint64(1)
    assert int(w[1, r]) >= 4 and bad_rows(b, w, b["pih"]) == [r] and bad_cycles(b, w) == []
    circ = c.circuit()
    assert set(np.flatnonzero(_oracle.plonk_gate_constraints_base(circ, w[:, r], b["cs"][:c.num_constants, r], b["pih"])).tolist()) == {1}
    # the top carry of a product's last column set to 1 (its limb with it): the sum constraint of that row fails, and the tie to zero
    top = c.u32_rows["add"][15]                                 # the first reduce's sixteenth column
    w = b["w"].copy()
    assert int(w[nn.ADD_ADDENDS + 2, top]) == 0
    w[nn.ADD_ADDENDS + 2, top] = 1
    w[nn.ADD_ADDENDS + 3 + 16, top] = 1
    assert bad_rows(b, w, b["pih"]) == [top]
    assert set(np.flatnonzero(_oracle.plonk_gate_constraints_base(circ, w[:, top], b["cs"][:c.num_constants, top], b["pih"])).tolist()) == {0}
    assert bad_cycles(b, w) == [next(cyc for cyc in c.cycles if (nn.ADD_ADDENDS + 2) * c.n + top in cyc)]


@pytest.mark.parametrize("tamper", ["a_word_of_Z_L", "a_claimed_x_limb"])
def test_tampered_inputs_are_refused_by_both_verifiers(tamper):
    b = honest(4)
    if tamper == "a_word_of_Z_L":
        rw = list(b["rw"])
        rw[5] ^= 1
        w, pis, _ = witness(b, rw=rw)
    else:
        ch = list(b["ch"])
        ch[3] ^= 1
        w, pis, _ = witness(b, ch=ch)
    assert prove_and_judge(b, w, pis) == (-210, 210)


@pytest.mark.parametrize("n", [1, 6, 0, 3])
def test_sizes_that_are_no_power_of_two_or_below_two_are_refused_at_build(n):
    with pytest.raises(ValueError):
        tr.SippTranscriptCircuit(n)


def test_challenges_of_and_check_obligations_read_the_records():
    b = build(4)
    d, c = b["npz"], b["c"]
    assert b["ch"] == [v for x, xi in b["ex"] for v in tc.limbs(x) + tc.limbs(xi)]
    check, holder = tr.check_obligations, c
    pis = c.public_inputs(b["st"], b["rw"], b["ch"])
    assert check(holder, pis, d["g1"], d["g2"], d["fq12"])
    for name, at in (("g1", 32), ("g2", 64 + 7), ("fq12", 192 + 3)):
        recs = {k: d[k].copy() for k in ("g1", "g2", "fq12")}
        recs[name][-1, at] ^= 1
        assert not check(holder, pis, recs["g1"], recs["g2"], recs["fq12"])
    assert not check(holder, pis[:-1], d["g1"], d["g2"], d["fq12"])


# ---- pinned shapes ------------------------------------------------------------------------------------------------------------------------
def shape_digests(n):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import outer_circuit_shapes as shapes
    b = build(n)
    c = b["c"]
    args = (b["st"], b["rw"], b["ch"])
    out = shapes.digests(c, args, args)
    out.update(rows_used=c.rows_used, log_n=c.log_n, n_levels=c.n_levels, n_public_inputs=c.n_pi, n_witness_inputs=len(c.in_cycle),
               n_input_cells=len(c.words_map()[0]), n_generators=len(c.generators()), n_transcript_rows=len(c.transcript_rows))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_shape_is_the_pinned_one(n):
    want = json.load(open(GOLDEN))["n%d" % n]
    got = shape_digests(n)
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []
