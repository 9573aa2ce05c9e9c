"""FRI fold chains in the outer circuit on the device: the ArithmeticExtension, Exponentiation and CosetInterpolation generators
(SIPP_GEN_ARITHMETIC_EXT / _EXPONENTIATION / _COSET_INTERPOLATION) on all three launch paths against the Python reading
(tests/_witness_reading.py, tests/_fri_fold_reading.py) cell for cell, the interpolation on thin levels both as the sixteen-lane scan and on one lane
(SIPP_ROUTE_WITNESS_INTERP_ONE_LANE); an opening proof made by the device read into FriFoldProver (sipp_amd/fri_fold.py), proved word for
word as the oracle proves the read witness, accepted by both verifiers, refused when tampered with."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import fri_fold as ff
from sipp_amd import merkle as mk
from tests import _fri_cases as fc
from tests import _fri_fold_reading as fr
from tests import _oracle
from tests import _witness_reading as rd
from tests._device import INTERP_ONE_LANE as ONE_LANE
from tests._device import NO_GRAPH, dev, first_mismatch, host, levels, run_levels
from tests.test_fri_fold_circuit import CASE_A4, CASE_A16
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

P = _oracle.P
W = 7
DIGEST = (81, 82, 83, 84)
NUM_WIRES, NUM_CONSTS = 135, 3
LAY = mk.SWAP_LAYOUT
# selector value -> generator; (s, d): 4 points in one chunk ... 16 points in 15; a chunk boundary on the last point ((2, 2), (4, 4), (4, 2)),
# a short last chunk ((3, 4), (4, 7)), no intermediate ((1, 2), (3, 8), (4, 16))
INTERP = {10: (1, 2), 11: (2, 2), 12: (3, 4), 13: (3, 8), 14: (4, 2), 15: (4, 4), 16: (4, 7), 17: (4, 16)}
ARITH, EXPO, SWAP, RACC, OTHER = 20, 21, 22, 23, 30
N_BITS = 64
GENS = ([(rd.GEN_COSET_INTERPOLATION, 0, v, s, d, W, 0, 0) for v, (s, d) in INTERP.items()] +
        [(rd.GEN_ARITHMETIC_EXT, 0, ARITH, 16, 1, 2, W, 0), (rd.GEN_EXPONENTIATION, 0, EXPO, N_BITS, 0, 0, 0, 0),
         (rd.GEN_POSEIDON_SWAP, 0, SWAP, LAY["in_"], LAY["out"], LAY["sbox"], LAY["swap"], LAY["delta"]),
         (rd.GEN_RANDOM_ACCESS, 0, RACC, 2, 22, 4, 0, 0)])
FOLD_GENS = GENS[:10]                       # the three new families alone
KINDS = list(INTERP) + [ARITH, EXPO, SWAP, RACC]


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)
    yield c
    c.close()


def table(rng, n, rows, kinds):
    """constants (selector column, two constant columns) and a random wire table; `rows` take the selector values `kinds` in turn, every
    other row OTHER.  The first rows of each kind carry the edge values: interpolation with shift = point = 0, with a point on the coset
    (a zero term), with values of p - 1; exponentiation with base 0, base p - 1 and a bit wire of 2; arithmetic on operands of p - 1."""
    consts = np.stack([np.full(n, OTHER, dtype=np.uint64), _oracle.rand_field(rng, n), _oracle.rand_field(rng, n)])
    rows = np.asarray(rows, dtype=np.int64)
    consts[0, rows] = np.array([kinds[k % len(kinds)] for k in range(len(rows))], dtype=np.uint64)
    w = _oracle.rand_field(rng, (NUM_WIRES, n))
    w[LAY["swap"]] = rng.integers(0, 2, size=n, dtype=np.uint64)
    seen = {}
    for r in rows:
        v = int(consts[0, r])
        k = seen[v] = seen.get(v, -1) + 1
        if v in INTERP:
            s = INTERP[v][0]
            m = 1 << s
            if k == 0:
                w[0, r], w[1 + 2 * m, r], w[2 + 2 * m, r] = 0, 0, 0
            elif k == 1:
                w[0, r], w[1 + 2 * m, r], w[2 + 2 * m, r] = 5, 5 * fr.domain(s)[0][m - 1] % P, 0
            elif k == 2:
                w[1:1 + 2 * m, r] = P - 1
                w[0, r] = P - 1
        elif v == EXPO:
            w[1:1 + N_BITS, r] = rng.integers(0, 2, size=N_BITS, dtype=np.uint64)
            if k == 0:
                w[0, r] = 0
            elif k == 1:
                w[0, r] = P - 1
            elif k == 2:
                w[7, r] = 2
            elif k == 3:
                w[1:1 + N_BITS, r] = _oracle.rand_field(rng, N_BITS)            # any field value in every bit wire
        elif v == ARITH and k == 0:
            w[:, r] = P - 1
            consts[1:, r] = P - 1
    return consts, w


def test_row_local_generators_match_the_reading(ctx):
    """sipp_plonk_generate_witness, one lane per row, 2^10 rows: every family's rows get the reading's cells; rows of another selector value
    stay as they were"""
    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(51)
    consts, w = table(rng, n, np.flatnonzero(np.arange(n) % 3 != 1), KINDS)
    want = rd.row_local(w, consts, GENS, None)
    other = consts[0] == OTHER
    assert other.sum() >= n // 3 and (want[:, other] == w[:, other]).all() and (want[:, ~other] != w[:, ~other]).any()
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, dev(consts), log_n, GENS)
    assert first_mismatch(host(d_w), want) is None


def test_wide_level_mixing_the_three_families_matches_the_reading(ctx):
    """one level of 16384 rows of a 2^15-row table (the one-lane level kernel) mixing the three families, launched one by one, captured, replayed"""
    log_n, n = 15, 1 << 15
    rng = np.random.default_rng(52)
    rows = np.flatnonzero(np.arange(n) % 2 == 0)
    assert len(rows) >= 16384
    consts, w = table(rng, n, rows, [k for k in KINDS if k not in (SWAP, RACC)])
    want = run_levels(ctx, w, consts, log_n, FOLD_GENS, levels([rows]), (NO_GRAPH, 0, 0))
    other = consts[0] == OTHER
    assert (want[:, other] == w[:, other]).all()


def test_thin_levels_mixing_interpolation_poseidon_and_short_rows_match_the_reading(ctx):
    """levels of 1, 2, 3, 4, 5 and 1024 rows (sixteen lanes per row, four rows per wave) in which interpolation rows of s = 1 .. 4 sit
    beside Poseidon-swap, arithmetic, exponentiation and RandomAccess rows: the sixteen-lane scan and the one-lane route give the
    reading's cells, launched one by one and replayed from the captured graph"""
    log_n, n = 12, 1 << 12
    rng = np.random.default_rng(53)
    perm = rng.permutation(n)
    sizes, level_rows, at = (1, 2, 3, 4, 5, 1024), [], 0
    for c in sizes:
        level_rows.append(np.sort(perm[at:at + c]))
        at += c
    kinds = [16, SWAP, 11, ARITH, 15, 10, EXPO, 12, RACC, 13, 14, 17]          # in turn: the level of one row is an interpolation row
    rows = np.concatenate(level_rows)
    consts, w = table(rng, n, rows, kinds)
    for c, r in zip(sizes, level_rows):                                        # every level holds an interpolation row, the others a mix
        held = set(int(v) for v in consts[0, r])
        assert held & set(INTERP) and (c == 1 or held - set(INTERP)), (c, held)
    assert set(int(v) for v in consts[0, level_rows[-1]]) == set(kinds)
    want = run_levels(ctx, w, consts, log_n, GENS, levels(level_rows), (NO_GRAPH, 0, 0, ONE_LANE, ONE_LANE, ONE_LANE | NO_GRAPH, 0))
    other = consts[0] == OTHER
    assert (want[:, other] == w[:, other]).all()


def test_bad_layouts_are_refused_and_the_ctx_still_generates(ctx):
    """a layout that leaves the table, s outside 1 .. 4, d < 2, n_bits outside 1 .. 64, n_ops = 0, W = 0: SIPP_E_BADARG before any launch"""
    import sipp_amd
    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(54)
    consts, w = table(rng, n, np.arange(n), KINDS)
    d_w, d_c = dev(w), dev(consts)
    I, A, E = rd.GEN_COSET_INTERPOLATION, rd.GEN_ARITHMETIC_EXT, rd.GEN_EXPONENTIATION
    bad = [(I, 0, 16, 0, 7, W, 0, 0), (I, 0, 16, 5, 7, W, 0, 0), (I, 0, 16, 4, 1, W, 0, 0), (I, 0, 16, 4, 0, W, 0, 0), (I, 0, 16, 4, 7, 0, 0, 0),
           (E, 0, EXPO, 0, 0, 0, 0, 0), (E, 0, EXPO, 65, 0, 0, 0, 0), (A, 0, ARITH, 0, 1, 2, W, 0), (A, 0, ARITH, 1, 1, 2, 0, 0),
           (A, 0, ARITH, 17, 1, 2, W, 0), (A, 0, ARITH, 1, 3, 2, W, 0), (A, 0, ARITH, 1, 1, 3, W, 0)]
    for g in bad:
        with pytest.raises(sipp_amd.SippError) as e:
            ctx.plonk_generate_witness(d_w, d_c, log_n, [g])
        assert e.value.code == -1, g
        assert (host(d_w) == w).all()
    # layouts that fit 135 wires leave a narrower table: interpolation (4, 2) needs 95 wires, 64 exponent bits 130
    narrow = np.ascontiguousarray(w[:94])
    d_n = dev(narrow)
    for g in ((I, 0, 14, 4, 2, W, 0, 0), (E, 0, EXPO, 64, 0, 0, 0, 0), (A, 0, ARITH, 12, 1, 2, W, 0)):
        with pytest.raises(sipp_amd.SippError) as e:
            ctx.plonk_generate_witness(d_n, d_c, log_n, [g])
        assert e.value.code == -1, g
        assert (host(d_n) == narrow).all()
    sched = sipp_amd.PlonkSchedule.from_dict(levels([np.arange(8)]))
    with pytest.raises(sipp_amd.SippError) as e:
        ctx.plonk_generate_witness_levels(d_w, d_c, log_n, [bad[1]], None, sched)
    assert e.value.code == -1 and (host(d_w) == w).all()
    ctx.plonk_generate_witness(d_w, d_c, log_n, GENS)
    assert first_mismatch(host(d_w), rd.row_local(w, consts, GENS, None)) is None


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _other_transcript(case):
    """the same oracles behind another transcript prefix: other challenges, other queries"""
    return fc.Case(case.id + "-second", log_n=case.log_n, rate_bits=case.rate_bits, cap_height=case.cap_height, widths=case.widths,
                   seed=case.seed, fri=case.fri, prefix=(9, 8, 7))


@pytest.fixture(scope="module", params=[CASE_A16, CASE_A4], ids=repr)
def opened(ctx, request):
    """two opening proofs made by the DEVICE (sipp_fri_prove_openings, equal to the oracle's word for word) and their fold data"""
    from tests.test_gpu_fri_edges import commit, prove_and_compare
    out = []
    for case in (request.param, _other_transcript(request.param)):
        inst = fc.build(case)
        devs, keep = commit(ctx, inst)
        pf, _ = prove_and_compare(ctx, inst, devs, fc.challenger(case))
        out.append(fr.fold_data(inst, pf))
        del devs, keep
    assert out[0][2] != out[1][2]
    fp = inst.fp
    return out, (inst.log_n + fp.rate_bits, fp.arity_bits[0], fp.n_rounds, len(out[0][1]), fp.num_queries)


@pytest.fixture(scope="module")
def prover(opened):
    import sipp_amd
    _, shape = opened
    fcirc = ff.FriFoldCircuit(*shape)
    ofp = fri(fcirc.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(fcirc.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(fcirc.log_n, C.byref(gp), C.byref(gfp), C.byref(gc))
    c = sipp_amd.Ctx(workspace_bytes=ws)
    pr = ff.FriFoldProver(c, *shape, fri=gfp, digest=DIGEST)
    yield pr, c, ofp
    pr.close()
    c.close()


def _verdicts(pr, ofp, pf):
    return pr.verify(pf), _oracle.plonk_verify_gates(pf, pr.cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST)


def test_folds_of_a_device_opening_proof_prove_and_verify(ctx, opened, prover):
    import sipp_amd
    data, _ = opened
    pr, c, ofp = prover
    fcirc = pr.circ
    cs = fcirc.constants_sigmas()
    assert (pr.cap == _oracle.Batch(cs, fcirc.log_n, rate_bits=3, cap_height=4).cap).all()
    L = sipp_amd.lib()
    for round_, args in enumerate(data):                           # the second opening proof goes through the same circuit data
        pis = fcirc.public_inputs(*args)
        pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
        pw = fcirc.partial_witness(*args)
        want = rd.replay(pw, cs[:6], fcirc.generators(), pih, fcirc.schedule())
        if round_ == 0:                                            # the device witness (the generation CircuitData.prove runs) = the reading
            sched = sipp_amd.PlonkSchedule.from_dict(fcirc.schedule())
            try:
                for route in (0, ONE_LANE):
                    assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
                    d_w = dev(pw)
                    ctx.plonk_generate_witness_levels(d_w, dev(cs[:6]), fcirc.log_n, fcirc.generators(), pih, sched)
                    assert first_mismatch(host(d_w), want) is None, route
            finally:
                assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
        pf = pr.prove(*args)
        ref = _oracle.plonk_prove_gates(want, cs, fcirc.log_n, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST, pis)
        assert len(pf) == len(ref) and (pf == ref).all(), round_
        assert _verdicts(pr, ofp, pf) == ((0, 0), 0)


@pytest.mark.parametrize("tamper", ["eval_elsewhere", "final_coefficient"])
def test_tampered_folds_are_refused_and_the_prover_goes_on(opened, prover, tamper):
    data, _ = opened
    pr, c, ofp = prover
    betas, final, queries = data[0]
    final, queries = list(final), [(x, old, [list(r) for r in ev]) for x, old, ev in queries]
    if tamper == "eval_elsewhere":
        x, old, ev = queries[2]
        j = (x & (pr.circ.arity - 1)) ^ 1                             # a point of round 0's coset that is not the opened one
        ev[0][j] = ((ev[0][j][0] + 1) % P, ev[0][j][1])
    else:
        final[1] = (final[1][0], (final[1][1] + 1) % P)
    pf = pr.prove(betas, final, queries)
    (st, stage), orc = _verdicts(pr, ofp, pf)
    assert st != 0 and orc != 0, (st, stage, orc)
    good = pr.prove(*data[0])
    assert _verdicts(pr, ofp, good) == ((0, 0), 0)
