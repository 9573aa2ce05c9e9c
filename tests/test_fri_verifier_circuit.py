"""The whole FRI query round in the outer circuit on the CPU (sipp_amd/fri_verifier.py): the Merkle, combination and fold wirings joined
on one builder, over opening proofs made by the oracle's FRI prover and read by tests/_fri_round_reading.py; the witness replayed level
by level (tests/_witness_reading.py), proved by the oracle and judged by both verifiers; the one reading of the index and of x per
query; the edges of the three shapes from the circuit's row lists; the pinned digests of
tests/golden/fri_verifier_circuit_shapes.json; the shapes that are refused at build."""
import json
import os
import sys

import numpy as np
import pytest

from sipp_amd import circuit as ci
from sipp_amd import fri_fold as ff
from sipp_amd import fri_initial as fi
from sipp_amd import fri_verifier as fv
from sipp_amd import merkle as mk
from tests import _fri_cases as fc
from tests import _fri_round_reading as rr
from tests import _merkle_reading as mr
from tests import _witness_reading as rd
from tests import _oracle, _verify
from tests.test_oracle_plonk import fri

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import outer_circuit_shapes as shapes  # noqa: E402

P = _oracle.P
DIGEST = (81, 82, 83, 84)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_verifier_circuit_shapes.json")
# leaves of at most 4 values (no leaf-hash rows), coset leaves of 32 values (four rows), coset trees of heights [5, 1]
ROUND_A16 = fc.Case("round-a16", log_n=10, rate_bits=1, cap_height=2, widths=(3, 2), seed=41,
                    fri=dict(arity_bits=4, final_poly_bits=2, num_queries=4))
# a 9-value leaf whose second row holds one value, coset leaves of 8 values (one full row), heights [7, 5, 3], batches of 11 and 9 columns
ROUND_A4_WIDE = fc.Case("round-a4-wide", log_n=10, rate_bits=1, cap_height=2, widths=(9, 2), seed=42,
                        fri=dict(arity_bits=2, final_poly_bits=4, num_queries=4))
# coset leaves of four values (no hash rows), six rounds of heights [5, 4, 3, 2, 1, 0]: the last tree has no sibling; a cap of 32
ROUND_A2_CAP = fc.Case("round-a2-cap", log_n=10, rate_bits=1, cap_height=5, widths=(5, 1), seed=43,
                       fri=dict(arity_bits=1, final_poly_bits=4, num_queries=3))
CASES = (ROUND_A16, ROUND_A4_WIDE, ROUND_A2_CAP)
# the circuit's arguments of every case: (log_m, cap_height, widths, batches, arity_bits, n_rounds, final_len, n_queries)
SHAPES = {"round-a16": (11, 2, [3, 2], [[0, 1, 2, 3, 4], [1, 3, 4]], 4, 2, 4, 4),
          "round-a4-wide": (11, 2, [9, 2], [list(range(11)), [1, 2, 3, 4, 5, 6, 7, 9, 10]], 2, 3, 16, 4),
          "round-a2-cap": (11, 5, [5, 1], [[0, 1, 2, 3, 4, 5], [1, 2, 3, 5]], 1, 6, 16, 3)}


# ---- the pinned shapes (tools/fri_verifier_circuit_shapes.py writes the file from shape_digests) -------------------------------------
def values(n, at):
    """n field values from position `at` of the fixed sequence p - 1, 0, 2, p - 1, 0, 5, ..."""
    return [(P - 1, 0, i)[i % 3] for i in range(at, at + n)]


def pairs(n, at):
    v = values(2 * n, at)
    return [(v[2 * i], v[2 * i + 1]) for i in range(n)]


def fixed_arguments(shape):
    """a fixed input of the shape: the largest index, the one with only the top bit set, 0, then small ones"""
    log_m, cap_height, widths, batches, arity_bits, n_rounds, final_len, n_queries = shape
    height = log_m - cap_height
    x = [((1 << log_m) - 1, 1 << (log_m - 1), 0, q % (1 << log_m))[min(q, 3)] for q in range(n_queries)]
    queries = [([values(w, q + o) for o, w in enumerate(widths)], [values(4 * height, q + o + 1) for o in range(len(widths))],
                [pairs(1 << arity_bits, q + r) for r in range(n_rounds)],
                [values(4 * (height - arity_bits * (r + 1)), q + r + 2) for r in range(n_rounds)]) for q in range(n_queries)]
    return (pairs(1, 0)[0], pairs(len(batches), 1), [pairs(len(b), 2 + k) for k, b in enumerate(batches)],
            [values(4 << cap_height, o) for o in range(len(widths))], [values(4 << cap_height, 3 + r) for r in range(n_rounds)],
            pairs(n_rounds, 4), pairs(final_len, 5), x, queries)


def shape_digests(shape):
    args = fixed_arguments(shape)
    return shapes.digests(fv.FriQueryRoundCircuit(*shape), args, args[:8])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_is_the_pinned_one(name):
    want = json.load(open(GOLDEN))[name]
    got = shape_digests(SHAPES[name])
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []


# ---- the circuit over the oracle's proofs ------------------------------------------------------------------------------------------
def build(case):
    inst = fc.build(case)
    pf = _oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, fc.challenger(case))
    args, shape, data = rr.round_data(inst, pf)
    assert shape == SHAPES[case.id]
    c = fv.FriQueryRoundCircuit(*shape)
    cs = c.constants_sigmas()
    cs_cap = _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap
    return {"case": case, "inst": inst, "proof": pf, "args": args, "data": data, "c": c, "cs": cs, "cs_cap": cs_cap}


@pytest.fixture(scope="module", params=CASES, ids=repr)
def joined(request):
    return build(request.param)


@pytest.fixture(scope="module")
def joined16():
    return build(ROUND_A16)


def witness(o, args=None):
    c = o["c"]
    args = o["args"] if args is None else args
    pis = c.public_inputs(*args[:8])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(c.partial_witness(*args), o["cs"][:c.num_constants], c.generators(), pih, c.schedule())
    return w, pis, pih


def satisfied(o, w, pih):
    c, circ = o["c"], o["c"].circuit()
    k = c.num_constants
    rows = [r for r in range(c.n) if _oracle.plonk_gate_constraints_base(circ, w[:, r], o["cs"][:k, r], pih).any()]
    flat = w.reshape(-1)
    cycles = [cyc for cyc in c.cycles if len(set(flat[np.asarray(cyc, dtype=np.int64)].tolist())) != 1]
    return rows, cycles


def prove_and_judge(o, w, pis):
    c = o["c"]
    op = _oracle.plonk_params(80, 8, 2)
    ofp = fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    circ = c.circuit()
    pf = _oracle.plonk_prove_gates(w, o["cs"], c.log_n, op, ofp, circ, DIGEST, pis)
    return _oracle.plonk_verify_gates(pf, o["cs_cap"], op, ofp, circ, DIGEST), _verify.lib_plonk_verify(pf, o["cs_cap"], op, ofp, circ, DIGEST)


def test_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(joined):
    o, c = joined, joined["c"]
    w, pis, pih = witness(o)
    assert satisfied(o, w, pih) == ([], [])
    assert (w[12:16, c.chain_row[-1]] == pih).all()
    assert prove_and_judge(o, w, pis) == (0, 0)


def test_input_cells_are_the_partial_witness_each_cell_once(joined):
    o, c = joined, joined["c"]
    cells, vals = c.input_cells(*o["args"])
    assert cells.dtype == vals.dtype == np.uint64 and cells.shape == vals.shape and len(set(cells.tolist())) == len(cells)
    w = np.zeros((c.num_wires, c.n), dtype=np.uint64)
    w.reshape(-1)[cells.astype(np.int64)] = vals
    assert (w == c.partial_witness(*o["args"])).all()
    # what the proof carries beyond the public inputs is witness input: rows, siblings, evaluations, coset siblings, indices
    log_m, cap_height, widths, _, a, R, _, Q = SHAPES[o["case"].id]
    h = log_m - cap_height
    per_query = 1 + sum(widths) + 4 * h * len(widths) + R * (2 << a) + R + 4 * sum(h - a * (r + 1) for r in range(R))
    assert len(c.in_cycle) == Q * per_query and len(c.pi_cycle) == c.n_pi
    # the caller's form of the data gives the same arguments
    cells2, vals2 = c.input_cells(*fv.proof_arguments(**o["data"]))
    assert (cells2 == cells).all() and (vals2 == vals).all()


def test_one_index_split_and_one_x_per_query(joined):
    """a BaseSum row per query and no other; the Exponentiation rows of base omega_M and the arithmetic op times the coset generator
    once per query; every path's swap wire, every RandomAccess bit wire and both exponents sit on the cycles of that split's bits"""
    o, c = joined, joined["c"]
    log_m, cap_height, widths, _, a, R, _, Q = SHAPES[o["case"].id]
    assert len(c.bs_row) == len(c.exp0_row) == len(c.x_row) == Q
    assert sorted(np.flatnonzero(c.gate == ci.BASE_SUM).tolist()) == sorted(c.bs_row)
    assert (c.gate == fv.EXPONENTIATION).sum() == Q * (1 + R)
    n = c.n
    cyc_of = {x: k for k, cyc in enumerate(c.cycles) for x in cyc}
    omega = cyc_of[0 * n + c.omega_row]
    assert sorted(r for r in np.flatnonzero(c.gate == fv.EXPONENTIATION).tolist() if cyc_of.get(0 * n + r) == omega) == sorted(c.exp0_row)
    h = log_m - cap_height
    for q in range(Q):
        bit = [cyc_of[(1 + i) * n + c.bs_row[q]] for i in range(log_m)]
        for o_ in range(len(widths)):
            assert [cyc_of[24 * n + r] for r in c.init_path_row[q][o_]] == bit[:h]
        for r in range(R):
            assert [cyc_of[24 * n + row] for row in c.coset_path_row[q][r]] == bit[a * (r + 1):h]
            ra = c.ra_row[q][r]
            for l in range(2):
                assert [cyc_of[(c.ra_stride * l + 2 + c.arity + t) * n + ra] for t in range(a)] == bit[a * r:a * (r + 1)]
        for ras in c.init_ra_row[q] + c.coset_ra_row[q]:
            for row in ras:
                for cp in range(c.cap_copies):
                    assert [cyc_of[(c.cap_stride * cp + 2 + c.n_cap + t) * n + row] for t in range(cap_height)] == bit[h:]
        assert [cyc_of[(1 + j) * n + c.exp0_row[q]] for j in range(log_m)] == bit[::-1]
        # x feeds the combination's denominators and the first shift
        x = cyc_of[6 * n + c.x_row[q]]
        assert all(cyc_of[0 * n + r] == x for r in c.den_row[q]) and cyc_of[2 * n + c.shift_row[q][0]] == x


def test_one_cell_per_evaluation_feeds_hash_interpolation_and_selection(joined):
    """limb l of evaluation j of a round: item j of RandomAccess copy l (natural order), value rev(j) of the interpolation row, input
    2 j + l of the coset leaf (the proof's order) -- one cycle"""
    o, c = joined, joined["c"]
    _, _, _, _, a, R, _, Q = SHAPES[o["case"].id]
    n, A = c.n, 1 << a
    cyc_of = {x: k for k, cyc in enumerate(c.cycles) for x in cyc}
    for q in range(Q):
        for r in range(R):
            for j in range(A):
                for l in range(2):
                    sel = cyc_of[(c.ra_stride * l + 2 + j) * n + c.ra_row[q][r]]
                    assert cyc_of[(1 + 2 * ff.reverse_bits(j, a) + l) * n + c.interp_row[q][r]] == sel
                    k = 2 * j + l
                    if c.coset_hash_row[q][r]:
                        assert cyc_of[(k % 8) * n + c.coset_hash_row[q][r][k // 8]] == sel
                    elif c.coset_path_row[q][r]:
                        assert cyc_of[k * n + c.coset_path_row[q][r][0]] == sel
                    else:                                   # height 0: the leaf is the cap selection's claimed words
                        row = c.coset_ra_row[q][r][k // c.cap_copies]
                        assert cyc_of[(c.cap_stride * (k % c.cap_copies) + 1) * n + row] == sel


def test_the_edges_of_the_shapes_are_reached():
    cs = {name: fv.FriQueryRoundCircuit(*shape) for name, shape in SHAPES.items()}
    c = cs["round-a16"]                                     # leaves of 3 and 2 values: no hash rows; coset leaves of 32: four rows
    assert all(hs == [[], []] for hs in c.init_hash_row) and all([len(h) for h in hs] == [4, 4] for hs in c.coset_hash_row)
    assert c.round_height == [5, 1] and [len(p) for p in c.coset_path_row[0]] == [5, 1] and [len(p) for p in c.init_path_row[0]] == [9, 9]
    c = cs["round-a4-wide"]                                 # 9 values: a second row holding one; 8 values: one full row
    assert all([len(h) for h in hs] == [2, 0] for hs in c.init_hash_row) and all([len(h) for h in hs] == [1, 1, 1] for hs in c.coset_hash_row)
    zero = next(cyc for cyc in c.cycles if 0 * c.n + c.zero_row in cyc)
    second = c.init_hash_row[0][0][1]
    first = c.init_hash_row[0][0][0]
    assert 0 * c.n + second not in zero                     # the ninth value
    assert all(t * c.n + second not in zero for t in range(1, 8))      # ... then the first row's outputs, not zero
    out_cycles = [next(cyc for cyc in c.cycles if (12 + t) * c.n + first in cyc) for t in range(1, 12)]
    assert all((t * c.n + second) in cyc for t, cyc in zip(range(1, 12), out_cycles))
    assert c.round_height == [7, 5, 3] and [len(b) for b in c.batches] == [11, 9]
    c = cs["round-a2-cap"]                                  # four values: no hash rows; the last tree is its cap
    assert all(hs == [[]] * 6 for hs in c.coset_hash_row) and c.round_height == [5, 4, 3, 2, 1, 0]
    assert all(p[5] == [] and len(p[4]) == 1 for p in c.coset_path_row) and c.n_cap == 32 and (c.cap_copies, c.cap_rows) == (2, 2)
    assert all([len(h) for h in hs] == [1, 0] for hs in c.init_hash_row)
    for c in cs.values():
        circ = c.circuit()
        assert circ["num_wires"] == 135 and circ["num_routed"] == 80 and len(c.generators()) <= 16
        assert [g[0] for g in c.generators()].count(ci.GEN_RANDOM_ACCESS) == 2
        for (si, row, lo, hi, off, nc) in circ["gates"]:
            d = max([len(f) for cn in mr.decode(circ["programs"], off, nc) for _, f in cn] or [0])
            assert (hi - lo - 1) + 1 + d <= 8 and lo <= row < hi
        assert max(max(cy) for cy in c.cycles) < 80 * c.n
        cells = [x for cy in c.cycles for x in cy]
        assert len(cells) == len(set(cells))


def test_out_of_scope_shapes_are_refused_at_build():
    shape = SHAPES["round-a16"]
    fv.FriQueryRoundCircuit(*shape, pow_bits=0, draw_challenges=False, n_salt=[0, 0])
    fv.FriQueryRoundCircuit(*shape[:4], [4, 4], *shape[5:])
    for kw in (dict(pow_bits=6), dict(draw_challenges=True), dict(n_salt=[0, 4])):
        with pytest.raises(AssertionError):
            fv.FriQueryRoundCircuit(*shape, **kw)
    with pytest.raises(AssertionError):
        fv.FriQueryRoundCircuit(*shape[:4], [4, 3], *shape[5:])                  # mixed arities
    with pytest.raises(AssertionError):
        fv.FriQueryRoundCircuit(*shape[:3], [[0, 1], []], *shape[4:])            # an empty batch
    with pytest.raises(AssertionError):
        fv.FriQueryRoundCircuit(11, 5, [5, 1], [[0]], 1, 7, 8, 1)                # a seventh round's tree would be smaller than its cap
    with pytest.raises(AssertionError):
        mk.MerkleOpeningCircuit(3, 0, 1, 1)                                      # the old class keeps its height >= 1


def test_the_three_modules_expose_their_wiring_and_the_old_classes_build():
    for mod, names in ((mk, ["opening_into"]), (fi, ["reduce_chain", "openings_into", "combine_into"]),
                       (ff, ["index_and_x", "fold_rounds_into", "final_poly_into"])):
        for name in names:
            assert callable(getattr(mod, name)), name
    assert mk.MerkleOpeningCircuit(3, 1, 1, 1).rows_used > 0
    assert fi.FriInitialCircuit(3, 1, [[0]], 1, k_base=1, k_ext=1).rows_used > 0
    assert ff.FriFoldCircuit(4, 1, 1, 1, 1).rows_used > 0


TAMPERS = ["row_value", "initial_sibling", "evaluation_not_at_within", "coset_sibling", "cap_word", "x_index", "beta", "final_coefficient",
           "opened_value"]


def tampered(args, what):
    """the arguments with one value moved by one"""
    alpha, points, opened, caps, round_caps, betas, final_poly, x, queries = args
    opened, betas, final_poly, x = [list(v) for v in opened], list(betas), list(final_poly), list(x)
    caps = [np.array(c, dtype=np.uint64) for c in caps]
    queries = [([list(r) for r in rows], [np.array(s, dtype=np.uint64) for s in sibs], [list(e) for e in evals],
                [np.array(s, dtype=np.uint64) for s in csibs]) for rows, sibs, evals, csibs in queries]
    bump = lambda p, l: tuple((v + (k == l)) % P for k, v in enumerate(p))
    if what == "row_value":
        queries[1][0][0][2] = (queries[1][0][0][2] + 1) % P
    elif what == "initial_sibling":
        queries[2][1][1][3, 0] = (int(queries[2][1][1][3, 0]) + 1) % P
    elif what == "evaluation_not_at_within":
        within = x[0] & 15
        j = (within + 5) % 16
        queries[0][2][0][j] = bump(queries[0][2][0][j], 1)
    elif what == "coset_sibling":
        queries[3][3][0][2, 1] = (int(queries[3][3][0][2, 1]) + 1) % P
    elif what == "cap_word":
        caps[1][x[0] >> 9, 2] = (int(caps[1][x[0] >> 9, 2]) + 1) % P
    elif what == "x_index":
        x[1] ^= 1
    elif what == "beta":
        betas[1] = bump(betas[1], 0)
    elif what == "final_coefficient":
        final_poly[3] = bump(final_poly[3], 1)
    else:
        opened[1][2] = bump(opened[1][2], 1)
    return (alpha, points, opened, caps, round_caps, betas, final_poly, x, queries)


@pytest.mark.parametrize("what", TAMPERS)
def test_tampered_inputs_give_proofs_both_verifiers_refuse(joined16, what):
    o = joined16
    args = tampered(o["args"], what)
    w, pis, pih = witness(o, args)
    rows, cycles = satisfied(o, w, pih)
    assert rows or cycles
    orc, lib = prove_and_judge(o, w, pis)
    assert orc != 0 and lib != 0, (orc, lib)
