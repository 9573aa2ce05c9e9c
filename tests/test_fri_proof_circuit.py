"""The whole of verify_fri_proof in the outer circuit on the CPU (sipp_amd/fri_proof.py): the challenger, the proof of work and the query
indices drawn in circuit, over opening proofs made by the oracle's FRI prover; the witness replayed level by level
(tests/_witness_reading.py with tests/_challenger_reading.py's kind 15), proved by the oracle and judged by both verifiers; the drawn
cells against the oracle's Challenger; the one split per query; the input map from the flat proof; tampering; the refusals; the pinned
digests of tests/golden/fri_proof_circuit_shapes.json (tools/fri_proof_circuit_shapes.py writes them)."""
import json
import os

import numpy as np
import pytest

from sipp_amd import circuit as ci
from sipp_amd import fri_proof as fp
from sipp_amd import fri_verifier as fv
from tests import _challenger_reading as cr
from tests import _fri_cases as fc
from tests import _fri_round_reading as rr
from tests import _merkle_reading as mr
from tests import _witness_reading as rd
from tests import _oracle
from tests.test_fri_verifier_circuit import ROUND_A2_CAP, ROUND_A4_WIDE, ROUND_A16, SHAPES, fixed_arguments, prove_and_judge, satisfied, shapes

P = _oracle.P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_proof_circuit_shapes.json")


def variant(case, tag, fri=None, **kw):
    return fc.Case(case.id + "-" + tag, log_n=case.log_n, rate_bits=case.rate_bits, cap_height=case.cap_height, widths=case.widths,
                   seed=case.seed, fri=dict(case.fri, **(fri or {})), **kw)


A16_RULE1 = variant(ROUND_A16, "rule1", dict(pow_rule=1))
A16_POW0 = variant(ROUND_A16, "pow0", dict(pow_bits=0))
A16_PREFIX8 = variant(ROUND_A16, "prefix8", prefix=range(1, 9))                  # nothing pending
A16_PENDING_OUT = variant(ROUND_A16, "pending-out", prefix=range(1, 10), gets=1)  # pending output that must be discarded
CASES = (ROUND_A16, ROUND_A4_WIDE, ROUND_A2_CAP, A16_RULE1, A16_POW0, A16_PREFIX8, A16_PENDING_OUT)


def shape_of(case):
    return SHAPES[case.id if case.id in SHAPES else "round-a16"]


def circuit_kw(case):
    return dict(pow_bits=case.fri["pow_bits"], pow_rule=case.fri["pow_rule"], n_in=len(cr.arriving(case)[0][1]))


def reading(case, shape, proof, transcript):
    log_m, cap_height, _, batches, arity_bits, n_rounds, final_len, n_queries = shape
    return cr.drawn(proof, transcript, log_m, cap_height, sum(len(b) for b in batches), arity_bits, n_rounds, final_len, n_queries,
                    case.fri["pow_rule"])


def arguments(c, proof, data, transcript):
    return fp.flat_proof_arguments(c, proof, data["caps"], data["points"], transcript)


def build(case):
    inst = fc.build(case)
    pf = _oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, fc.challenger(case))
    _, shape, data = rr.round_data(inst, pf)
    assert shape == shape_of(case)
    transcript, pending_out = cr.arriving(case)
    c = fp.FriProofCircuit(*shape, **circuit_kw(case))
    cs = c.constants_sigmas()
    cs_cap = _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap
    return {"case": case, "inst": inst, "proof": pf, "data": data, "transcript": transcript, "pending_out": pending_out, "c": c, "cs": cs,
            "cs_cap": cs_cap, "args": arguments(c, pf, data, transcript), "drawn": reading(case, shape, pf, transcript)}


@pytest.fixture(scope="module", params=CASES, ids=repr)
def whole(request):
    return build(request.param)


@pytest.fixture(scope="module")
def whole16():
    return build(ROUND_A16)


def witness(o, args=None):
    if args is None:                                            # the good witness of a case: replayed once
        if "witness" not in o:
            o["witness"] = witness(o, o["args"])
        return o["witness"]
    c = o["c"]
    pis = c.public_inputs(*args[:6])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(c.partial_witness(*args), o["cs"][:c.num_constants], c.generators(), pih, c.schedule())
    return w, pis, pih


def test_the_cases_reach_what_they_are_for():
    assert [len(cr.arriving(c)[0][1]) for c in CASES] == [3, 3, 3, 3, 3, 0, 0]
    assert [len(cr.arriving(c)[1]) for c in CASES] == [0, 0, 0, 0, 0, 8, 7]
    assert ci._i64(1 << 63) < 0 and ci._i64(1 << 63) % P == 1 << 63             # the top limb's coefficient in the int64 program words
    assert cr.GEN_BASE_SUM == ci.GEN_BASE_SUM


def test_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(whole):
    o, c = whole, whole["c"]
    w, pis, pih = witness(o)
    assert satisfied(o, w, pih) == ([], [])
    assert (w[12:16, c.chain_row[-1]] == pih).all()
    assert prove_and_judge(o, w, pis) == (0, 0)


def test_the_drawn_cells_hold_the_readings_values(whole):
    o, c, d = whole, whole["c"], whole["drawn"]
    w, _, _ = witness(o)
    at = lambda cell: int(w[cell[0], cell[1]])
    limbs = lambda row: [int(v) for v in w[1:65, row]]
    bits = lambda v: [(v >> i) & 1 for i in range(64)]
    assert tuple(at(x) for x in c.alpha_cells) == d["alpha"]
    assert [tuple(at(x) for x in b) for b in c.beta_cells] == d["betas"]
    assert at(c.response_cell) == d["response"] and limbs(c.pow_row) == bits(d["response"])
    assert limbs(c.pow_row)[64 - c.pow_bits:] == [0] * c.pow_bits
    assert [at(x) for x in c.index_cells] == d["challenges"]
    assert [limbs(r) for r in c.bs_row] == [bits(v) for v in d["challenges"]]
    assert [sum(b << i for i, b in enumerate(limbs(r)[:c.log_m])) for r in c.bs_row] == d["x_index"]
    assert [int(w[0, r]) for r in c.cap_sum_row] == d["cap_index"]
    assert [[int(w[0, r]) for r in rows] for rows in c.within_row] == d["within"]
    # what the query-round reading drew on the host is what the circuit drew
    args, _, _ = rr.round_data(o["inst"], o["proof"])
    assert d["alpha"] == args[0] and d["betas"] == args[5] and d["x_index"] == args[7]


def test_one_split_per_query_serves_every_consumer(whole):
    """a 64-limb split per query and one for the response, no other; no split of a recombined index: the low log_m limbs sit on the
    cycles of every path's swap wire, every RandomAccess bit wire, the exponent and the limbs of the kind-15 rows, whose sums are the
    RandomAccess indices"""
    o, c = whole, whole["c"]
    log_m, cap_height, widths, _, a, R, _, Q = shape_of(o["case"])
    assert sorted(np.flatnonzero(c.gate == fp.BASE_SPLIT64).tolist()) == sorted(c.bs_row + [c.pow_row]) and len(c.bs_row) == Q
    assert not (c.gate == ci.BASE_SUM).any()
    assert (c.gate == fp.BASE_SUM_CAP).sum() == Q and (c.gate == fp.BASE_SUM_WITHIN).sum() == Q * R
    gens = {g[2]: g for g in c.generators()}
    assert gens[fp.BASE_SPLIT64][0] == ci.GEN_BASE_SPLIT and gens[fp.BASE_SPLIT64][3:5] == (64, 1)
    assert gens[fp.BASE_SUM_CAP][0] == gens[fp.BASE_SUM_WITHIN][0] == ci.GEN_BASE_SUM
    assert gens[fp.BASE_SUM_CAP][3:5] == (cap_height, 1) and gens[fp.BASE_SUM_WITHIN][3:5] == (a, 1)
    n = c.n
    cyc_of = {x: k for k, cyc in enumerate(c.cycles) for x in cyc}
    h = log_m - cap_height
    zero = cyc_of[0 * n + c.zero_row]
    assert [cyc_of.get((64 - k) * n + c.pow_row) == zero for k in range(64)] == [k < c.pow_bits for k in range(64)]
    inputs = {x for cyc in c.pi_cycle + c.in_cycle for x in cyc}
    for q in range(Q):
        bit = [cyc_of[(1 + i) * n + c.bs_row[q]] for i in range(log_m)]
        assert cyc_of[0 * n + c.bs_row[q]] == cyc_of[c.index_cells[q][0] * n + c.index_cells[q][1]]
        for o_ in range(len(widths)):
            assert [cyc_of[24 * n + r] for r in c.init_path_row[q][o_]] == bit[:h]
        cap = c.cap_sum_row[q]
        assert [cyc_of[(1 + t) * n + cap] for t in range(cap_height)] == bit[h:]
        for r in range(R):
            assert [cyc_of[24 * n + row] for row in c.coset_path_row[q][r]] == bit[a * (r + 1):h]
            ra, ws = c.ra_row[q][r], c.within_row[q][r]
            assert [cyc_of[(1 + t) * n + ws] for t in range(a)] == bit[a * r:a * (r + 1)]
            for l in range(2):
                assert [cyc_of[(c.ra_stride * l + 2 + c.arity + t) * n + ra] for t in range(a)] == bit[a * r:a * (r + 1)]
                assert cyc_of[c.ra_stride * l * n + ra] == cyc_of[0 * n + ws] and c.ra_stride * l * n + ra not in inputs
        for ras in c.init_ra_row[q] + c.coset_ra_row[q]:
            for row in ras:
                for cp in range(c.cap_copies):
                    assert [cyc_of[(c.cap_stride * cp + 2 + c.n_cap + t) * n + row] for t in range(cap_height)] == bit[h:]
                    assert cyc_of[c.cap_stride * cp * n + row] == cyc_of[0 * n + cap] and c.cap_stride * cp * n + row not in inputs
        assert [cyc_of[(1 + j) * n + c.exp0_row[q]] for j in range(log_m)] == bit[::-1]
    # alpha and the betas feed their consumers from the challenger's rows: no input cell holds them
    for cell in list(c.alpha_cells) + [x for b in c.beta_cells for x in b] + c.index_cells + [c.response_cell]:
        assert cell[1] in c.transcript_row + c.pow_hash_row and cell[0] * n + cell[1] not in inputs
    assert len(c.pow_hash_row) == o["case"].fri["pow_rule"]
    circ = c.circuit()
    for (si, row, lo, hi, off, nc) in circ["gates"]:
        d = max([len(f) for cn in mr.decode(circ["programs"], off, nc) for _, f in cn] or [0])
        assert (hi - lo - 1) + 1 + d <= 8 and lo <= row < hi
    assert len(c.generators()) <= 16


def test_the_input_map_reads_every_input_from_its_proof_word(whole):
    o, c = whole, whole["c"]
    cells, word = c.input_map()
    assert cells.dtype == np.uint64 and cells.shape == word.shape and len(set(cells.tolist())) == len(cells)
    assert len(o["proof"]) == c.proof_words and word.min() >= 8 and word.max() == c.proof_words - 1
    # every witness-input cycle is covered exactly once, and of the public inputs exactly those the proof carries
    have = sorted(cells.tolist())
    carried = [t for t in range(c.n_pi) if t >= c.pi_rounds or any(c.pi_opened(b, 0, 0) <= t < c.pi_opened(b, len(cols), 0)
                                                                   for b, cols in enumerate(c.batches))]
    assert have == sorted(x for cyc in c.in_cycle + [c.pi_cycle[t] for t in carried] for x in cyc)
    # a probe proof whose word k holds k + 1: the gathered values are word_index + 1, and they are what the arguments put there
    probe = np.arange(1, c.proof_words + 1, dtype=np.uint64)
    data = o["data"]
    pcells, pvals, ppis = c.proof_inputs(probe, data["caps"], data["points"], o["transcript"])
    assert (pcells[:len(cells)] == cells).all() and (pvals[:len(cells)] == (word + 1).astype(np.uint64)).all()
    pargs = arguments(c, probe, data, o["transcript"])
    assert [int(v) for v in ppis] == c.public_inputs(*pargs[:6])
    w = np.zeros((c.num_wires, c.n), dtype=np.uint64)
    w.reshape(-1)[pcells.astype(np.int64)] = pvals
    assert len(set(pcells.tolist())) == len(pcells) and (w == c.partial_witness(*pargs)).all()
    # a real proof: the partial witness that prove(*arguments) builds
    gcells, gvals, gpis = c.proof_inputs(o["proof"], data["caps"], data["points"], o["transcript"])
    w = np.zeros((c.num_wires, c.n), dtype=np.uint64)
    w.reshape(-1)[gcells.astype(np.int64)] = gvals
    assert (w == c.partial_witness(*o["args"])).all() and [int(v) for v in gpis] == c.public_inputs(*o["args"][:6])
    acells, avals = c.input_cells(*o["args"])
    assert sorted(zip(acells.tolist(), avals.tolist())) == sorted(zip(gcells.tolist(), gvals.tolist()))


TAMPERS = ["row_value", "initial_sibling", "evaluation_not_at_within", "coset_sibling", "cap_word", "final_coefficient", "opened_value",
           "round_cap_word", "transcript_word", "pow_witness"]


def tampered(o, what):
    """the arguments with one value moved by one (the proof-of-work witness: to the nearest invalid one)"""
    transcript, points, opened, caps, round_caps, final_poly, pow_witness, queries = o["args"]
    x = o["drawn"]["x_index"]
    transcript = (list(transcript[0]), list(transcript[1]))
    opened, final_poly = [list(v) for v in opened], list(final_poly)
    caps, round_caps = [np.array(c, dtype=np.uint64).reshape(-1, 4) for c in caps], [np.array(c, dtype=np.uint64).reshape(-1, 4) for c in round_caps]
    queries = [([list(r) for r in rows], [np.array(s, dtype=np.uint64).reshape(-1, 4) for s in sibs], [list(e) for e in evals],
                [np.array(s, dtype=np.uint64).reshape(-1, 4) for s in csibs]) for rows, sibs, evals, csibs in queries]
    bump = lambda p, l: tuple((v + (k == l)) % P for k, v in enumerate(p))
    if what == "row_value":
        queries[1][0][0][2] = (queries[1][0][0][2] + 1) % P
    elif what == "initial_sibling":
        queries[2][1][1][3, 0] = (int(queries[2][1][1][3, 0]) + 1) % P
    elif what == "evaluation_not_at_within":
        j = ((x[0] & 15) + 5) % 16
        queries[0][2][0][j] = bump(queries[0][2][0][j], 1)
    elif what == "coset_sibling":
        queries[3][3][0][2, 1] = (int(queries[3][3][0][2, 1]) + 1) % P
    elif what == "cap_word":
        caps[1][x[0] >> 9, 2] = (int(caps[1][x[0] >> 9, 2]) + 1) % P
    elif what == "final_coefficient":
        final_poly[3] = bump(final_poly[3], 1)
    elif what == "opened_value":
        opened[1][2] = bump(opened[1][2], 1)
    elif what == "round_cap_word":                              # beta_1 moves, and everything drawn after it
        round_caps[1][3, 1] = (int(round_caps[1][3, 1]) + 1) % P
    elif what == "transcript_word":
        transcript[0][9] = (transcript[0][9] + 1) % P           # a capacity word: nothing overwrites it
    else:
        shape = shape_of(o["case"])
        pow_witness = cr.invalid_witness(o["proof"], o["transcript"], shape[1], sum(len(b) for b in shape[3]), shape[5], shape[6],
                                         o["case"].fri["pow_rule"], o["case"].fri["pow_bits"])
    return (transcript, points, opened, caps, round_caps, final_poly, pow_witness, queries)


@pytest.mark.parametrize("what", TAMPERS)
def test_tampered_inputs_give_proofs_both_verifiers_refuse(whole16, what):
    o = whole16
    args = tampered(o, what)
    w, pis, pih = witness(o, args)
    rows, cycles = satisfied(o, w, pih)
    assert rows or cycles
    orc, lib = prove_and_judge(o, w, pis)
    assert orc != 0 and lib != 0, (orc, lib)


def test_an_invalid_witness_under_rule_1_is_refused():
    o = build(A16_RULE1)
    w, pis, pih = witness(o, tampered(o, "pow_witness"))
    rows, cycles = satisfied(o, w, pih)
    assert rows == [] and len(cycles) == 1 and o["c"].n * 0 + o["c"].zero_row in cycles[0]      # only the leading zeros fail
    orc, lib = prove_and_judge(o, w, pis)
    assert orc != 0 and lib != 0, (orc, lib)


def test_out_of_scope_shapes_are_refused_at_build():
    shape = SHAPES["round-a16"]
    fp.FriProofCircuit(*shape, pow_bits=32, pow_rule=1, n_in=7, n_salt=[0, 0])
    fp.FriProofCircuit(*shape[:4], [4, 4], *shape[5:])
    for kw in (dict(pow_bits=33), dict(n_in=8), dict(pow_rule=2), dict(n_salt=[0, 4])):
        with pytest.raises(AssertionError):
            fp.FriProofCircuit(*shape, **kw)
    with pytest.raises(AssertionError):
        fp.FriProofCircuit(*shape[:4], [4, 3], *shape[5:])                       # mixed arities
    with pytest.raises(AssertionError):
        fp.FriProofCircuit(*shape[:3], [[0, 1], []], *shape[4:])                 # an empty batch
    # the query-round circuit still takes neither the proof of work nor the challenger
    for kw in (dict(pow_bits=6), dict(draw_challenges=True)):
        with pytest.raises(AssertionError):
            fv.FriQueryRoundCircuit(*shape, **kw)


# ---- the pinned shapes (tools/fri_proof_circuit_shapes.py writes the file from shape_digests) ------------------------------------------
PINNED = {"round-a16": dict(pow_bits=6, pow_rule=0, n_in=3), "round-a4-wide": dict(pow_bits=6, pow_rule=0, n_in=3),
          "round-a2-cap": dict(pow_bits=6, pow_rule=0, n_in=3), "round-a16-rule1": dict(pow_bits=6, pow_rule=1, n_in=3),
          "round-a16-pow0-prefix8": dict(pow_bits=0, pow_rule=0, n_in=0), "round-a16-pow32-in7": dict(pow_bits=32, pow_rule=0, n_in=7)}


def shape_digests(name):
    shape = SHAPES[name if name in SHAPES else "round-a16"]
    c = fp.FriProofCircuit(*shape, **PINNED[name])
    _, points, opened, caps, round_caps, _, final_poly, _, queries = fixed_arguments(shape)
    transcript = ([(P - 1, 0, 7 + t)[t % 3] for t in range(12)], [P - 2 - t for t in range(c.n_in)])
    args = (transcript, points, opened, caps, round_caps, final_poly, P - 3, queries)
    return shapes.digests(c, args, args[:6])


@pytest.mark.parametrize("name", sorted(PINNED))
def test_shape_is_the_pinned_one(name):
    want = json.load(open(GOLDEN))[name]
    got = shape_digests(name)
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []
