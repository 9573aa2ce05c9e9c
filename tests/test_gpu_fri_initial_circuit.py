"""FRI's initial combination in the outer circuit on the device: the ReducingExtension and quotient generators (SIPP_GEN_REDUCING_EXT /
_QUOTIENT_EXT) and the base Reducing generator on all three launch paths against the Python reading (tests/_witness_reading.py)
cell for cell, the reducing rows on thin levels both as the sixteen-lane scan and on one lane (SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE); an
opening proof made by the device read into FriInitialProver (sipp_amd/fri_initial.py), proved word for word as the oracle proves the
read witness, accepted by both verifiers, refused when tampered with."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import fri_initial as fi
from sipp_amd import merkle as mk
from tests import _fri_cases as fc
from tests import _fri_fold_reading as fr
from tests import _fri_initial_reading as ir
from tests import _oracle
from tests import _witness_reading as rd
from tests._device import INTERP_ONE_LANE, NO_GRAPH, REDUCE_ONE_LANE, dev, first_mismatch, host, levels, run_levels
from tests.test_fri_fold_circuit import CASE_A4, CASE_A16
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

P = _oracle.P
W = 7
DIGEST = (95, 96, 97, 98)
NUM_WIRES, NUM_CONSTS = 135, 3
LAY = mk.SWAP_LAYOUT
# selector value -> K: one coefficient, fewer than / exactly / more than sixteen (one lane idle ... two per lane), the widest that fit 135 wires
RED = {40: 1, 41: 2, 42: 15, 43: 16, 44: 17, 45: 25, 46: 43}
REDX = {50: 1, 51: 16, 52: 17, 53: 19, 54: 32}
QUOT, QUOT_W4, INTERP, ARITH, EXPO, SWAP, RACC, OTHER = 60, 61, 16, 20, 21, 22, 23, 30
N_BITS = 64
RED_GENS = [(rd.GEN_REDUCING, 0, v, K, W, 0, 0, 0) for v, K in RED.items()]
REDX_GENS = [(rd.GEN_REDUCING_EXT, 0, v, K, W, 0, 0, 0) for v, K in REDX.items()]
QUOT_GENS = [(rd.GEN_QUOTIENT_EXT, 0, QUOT, 16, 1, 2, W, 0), (rd.GEN_QUOTIENT_EXT, 0, QUOT_W4, 1, 1, 2, 4, 0)]
OLD_GENS = [(rd.GEN_COSET_INTERPOLATION, 0, INTERP, 4, 7, W, 0, 0),
            (rd.GEN_POSEIDON_SWAP, 0, SWAP, LAY["in_"], LAY["out"], LAY["sbox"], LAY["swap"], LAY["delta"]),
            (rd.GEN_ARITHMETIC_EXT, 0, ARITH, 16, 1, 2, W, 0), (rd.GEN_EXPONENTIATION, 0, EXPO, N_BITS, 0, 0, 0, 0),
            (rd.GEN_RANDOM_ACCESS, 0, RACC, 2, 22, 4, 0, 0)]
# the level entry point takes at most 16 generators: the base reductions in one call, the extension reductions in another, both beside
# the quotient, interpolation and Poseidon-swap rows
CALL_A = RED_GENS + QUOT_GENS + OLD_GENS                # 7 + 2 + 5
CALL_B = REDX_GENS + QUOT_GENS + OLD_GENS               # 5 + 2 + 5
ALL_GENS = RED_GENS + REDX_GENS + QUOT_GENS + OLD_GENS
KINDS_A, KINDS_B, KINDS_ALL = ([g[2] for g in gs] for gs in (CALL_A, CALL_B, ALL_GENS))


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)
    yield c
    c.close()


def table(rng, n, rows, kinds):
    """constants (selector column, two constant columns) and a random wire table; `rows` take the selector values `kinds` in turn, every
    other row OTHER.  The first rows of each kind carry the edge values: reductions with alpha = 0, with alpha = (p - 1, p - 1), with an
    old accumulator and coefficients of p - 1; quotients with a zero denominator, with c0 = 0, and (W = 4) with a = (2, 1), whose norm
    is zero; interpolation with shift = point = 0.  Also returns the quotient rows that have no inverse."""
    consts = np.stack([np.full(n, OTHER, dtype=np.uint64), _oracle.rand_field(rng, n), _oracle.rand_field(rng, n)])
    rows = np.asarray(rows, dtype=np.int64)
    consts[0, rows] = np.array([kinds[k % len(kinds)] for k in range(len(rows))], dtype=np.uint64)
    w = _oracle.rand_field(rng, (NUM_WIRES, n))
    w[LAY["swap"]] = rng.integers(0, 2, size=n, dtype=np.uint64)
    seen, no_inverse = {}, []
    for r in rows:
        v = int(consts[0, r])
        k = seen[v] = seen.get(v, -1) + 1
        if v in RED or v in REDX:
            K = RED[v] if v in RED else 2 * REDX[v]
            if k == 0:
                w[0:2, r] = 0
            elif k == 1:
                w[0:2, r] = P - 1
            elif k == 2:
                w[2:4 + K, r] = P - 1
        elif v == QUOT:
            if k == 0:
                w[0:2, r] = 0
            elif k == 1:
                consts[1, r] = 0
            elif k == 2:
                w[:, r] = P - 1
            if k < 2:
                no_inverse.append(int(r))
        elif v == QUOT_W4 and k == 0:
            w[0, r], w[1, r] = 2, 1
            no_inverse.append(int(r))
        elif v == INTERP and k == 0:
            w[0, r], w[33, r], w[34, r] = 0, 0, 0
        elif v == EXPO:
            w[1:1 + N_BITS, r] = rng.integers(0, 2, size=N_BITS, dtype=np.uint64)
    return consts, w, no_inverse


def test_row_local_generators_match_the_reading(ctx):
    """sipp_plonk_generate_witness, one lane per row, 2^10 rows: the rows of kinds 7, 13 and 14 beside the older families get the
    reading's cells; rows of another selector value stay as they were; the quotient edge rows write (0, 0)"""
    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(71)
    consts, w, no_inverse = table(rng, n, np.flatnonzero(np.arange(n) % 3 != 1), KINDS_ALL)
    want = rd.row_local(w, consts, ALL_GENS, None)
    other = consts[0] == OTHER
    assert other.sum() >= n // 3 and (want[:, other] == w[:, other]).all() and (want[:, ~other] != w[:, ~other]).any()
    assert len(no_inverse) == 3 and (want[2:4, no_inverse] == 0).all() and (w[2:4, no_inverse] != 0).all()
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, dev(consts), log_n, ALL_GENS)
    assert first_mismatch(host(d_w), want) is None


@pytest.mark.parametrize("call", ["base", "ext"])
def test_wide_level_matches_the_reading(ctx, call):
    """one level of 16384 rows of a 2^15-row table (the one-lane level kernel) mixing the reductions, the quotient and arithmetic rows,
    launched one by one, captured, replayed"""
    log_n, n = 15, 1 << 15
    rng = np.random.default_rng(72)
    rows = np.flatnonzero(np.arange(n) % 2 == 0)
    assert len(rows) >= 16384
    gens = (RED_GENS if call == "base" else REDX_GENS) + QUOT_GENS + OLD_GENS[2:3]
    consts, w, _ = table(rng, n, rows, [g[2] for g in gens])
    want = run_levels(ctx, w, consts, log_n, gens, levels([rows]), (NO_GRAPH, 0, 0))
    other = consts[0] == OTHER
    assert (want[:, other] == w[:, other]).all()


@pytest.mark.parametrize("call", ["base", "ext"])
def test_thin_levels_mixing_reductions_quotients_interpolation_and_poseidon_match_the_reading(ctx, call):
    """levels of 1, 2, 3, 4, 5 and 1024 rows (sixteen lanes per row, four rows per wave) in which reducing rows of every K sit beside
    quotient, interpolation, Poseidon-swap and short rows: the sixteen-lane scan and the one-lane route give the reading's cells,
    launched one by one and replayed from the captured graph"""
    log_n, n = 12, 1 << 12
    rng = np.random.default_rng(73)
    perm = rng.permutation(n)
    sizes, level_rows, at = (1, 2, 3, 4, 5, 1024), [], 0
    for c in sizes:
        level_rows.append(np.sort(perm[at:at + c]))
        at += c
    gens, red = (CALL_A, RED) if call == "base" else (CALL_B, REDX)
    assert len(gens) <= 16
    # in turn, so that the small levels hold a reducing row each and a wave mixes the families
    others = [g[2] for g in gens if g[2] not in red]
    kinds = [v for pair in zip(red, others) for v in pair] + others[len(red):]
    assert sorted(kinds) == sorted(g[2] for g in gens)
    rows = np.concatenate(level_rows)
    consts, w, no_inverse = table(rng, n, rows, kinds)
    for c, r in zip(sizes, level_rows):
        held = set(int(v) for v in consts[0, r])
        assert held & set(red) and (c == 1 or held - set(red)), (c, held)
    assert set(int(v) for v in consts[0, level_rows[-1]]) == set(kinds)
    routes = (0, NO_GRAPH, REDUCE_ONE_LANE, REDUCE_ONE_LANE | INTERP_ONE_LANE, REDUCE_ONE_LANE | NO_GRAPH, 0)
    want = run_levels(ctx, w, consts, log_n, gens, levels(level_rows), routes)
    other = consts[0] == OTHER
    assert (want[:, other] == w[:, other]).all()
    assert len(no_inverse) == 3 and (want[2:4, no_inverse] == 0).all() and (w[2:4, no_inverse] != 0).all()


def test_bad_layouts_are_refused_and_the_ctx_still_generates(ctx):
    """K = 0, 4 + 4K > num_wires, W = 0, n_ops = 0, a constant column out of range: SIPP_E_BADARG before any launch"""
    import sipp_amd
    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(74)
    consts, w, _ = table(rng, n, np.arange(n), KINDS_ALL)
    d_w, d_c = dev(w), dev(consts)
    X, Q = rd.GEN_REDUCING_EXT, rd.GEN_QUOTIENT_EXT
    bad = [(X, 0, 50, 0, W, 0, 0, 0), (X, 0, 50, 33, W, 0, 0, 0), (X, 0, 50, 1 << 30, W, 0, 0, 0), (X, 0, 50, 19, 0, 0, 0, 0),
           (Q, 0, QUOT, 0, 1, 2, W, 0), (Q, 0, QUOT, 17, 1, 2, W, 0), (Q, 0, QUOT, 1, 3, 2, W, 0), (Q, 0, QUOT, 1, 1, 3, W, 0),
           (Q, 0, QUOT, 1, 1, 2, 0, 0), (X, 3, 50, 1, W, 0, 0, 0)]
    for g in bad:
        with pytest.raises(sipp_amd.SippError) as e:
            ctx.plonk_generate_witness(d_w, d_c, log_n, [g])
        assert e.value.code == -1, g
        assert (host(d_w) == w).all()
    # a layout that fits 135 wires leaves a narrower table: K = 19 needs 80 wires
    narrow = np.ascontiguousarray(w[:79])
    d_n = dev(narrow)
    for g in ((X, 0, 53, 19, W, 0, 0, 0), (Q, 0, QUOT, 10, 1, 2, W, 0)):
        with pytest.raises(sipp_amd.SippError) as e:
            ctx.plonk_generate_witness(d_n, d_c, log_n, [g])
        assert e.value.code == -1, g
        assert (host(d_n) == narrow).all()
    sched = sipp_amd.PlonkSchedule.from_dict(levels([np.arange(8)]))
    with pytest.raises(sipp_amd.SippError) as e:
        ctx.plonk_generate_witness_levels(d_w, d_c, log_n, [bad[0]], None, sched)
    assert e.value.code == -1 and (host(d_w) == w).all()
    ctx.plonk_generate_witness(d_w, d_c, log_n, ALL_GENS)
    assert first_mismatch(host(d_w), rd.row_local(w, consts, ALL_GENS, None)) is None


def test_the_route_setter_takes_the_new_bit_and_no_unknown_one(ctx):
    import sipp_amd
    L = sipp_amd.lib()
    try:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, REDUCE_ONE_LANE) == 0
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 8) == -1
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 64) == -1
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 1 | 2 | 4 | 16 | 32) == 0
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _other_transcript(case):
    """the same oracles behind another transcript prefix: other challenges, other queries"""
    return fc.Case(case.id + "-second", log_n=case.log_n, rate_bits=case.rate_bits, cap_height=case.cap_height, widths=case.widths,
                   seed=case.seed, fri=case.fri, prefix=(9, 8, 7))


# chains of three rows with a padded first row on one case, the widest rows on the other
@pytest.fixture(scope="module", params=[(CASE_A16, (2, 2)), (CASE_A4, (None, None))], ids=lambda p: repr(p[0]))
def opened(ctx, request):
    """two opening proofs made by the DEVICE (sipp_fri_prove_openings, equal to the oracle's word for word) and their data"""
    from tests.test_gpu_fri_edges import commit, prove_and_compare
    case0, ks = request.param
    out = []
    for case in (case0, _other_transcript(case0)):
        inst = fc.build(case)
        devs, keep = commit(ctx, inst)
        pf, _ = prove_and_compare(ctx, inst, devs, fc.challenger(case))
        alpha, points, vals, queries, batches, n_columns = ir.initial_data(inst, pf)
        assert [q[2] for q in queries] == [q[1] for q in fr.fold_data(inst, pf)[2]]          # the link to the fold circuit
        out.append((alpha, points, vals, queries))
        del devs, keep
    assert out[0][3] != out[1][3]
    fp = inst.fp
    return out, (inst.log_n + fp.rate_bits, n_columns, batches, fp.num_queries), ks


@pytest.fixture(scope="module")
def prover(opened):
    import sipp_amd
    _, shape, ks = opened
    circ = fi.FriInitialCircuit(*shape, k_base=ks[0], k_ext=ks[1])
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc))
    c = sipp_amd.Ctx(workspace_bytes=ws)
    pr = fi.FriInitialProver(c, *shape, fri=gfp, digest=DIGEST, k_base=ks[0], k_ext=ks[1])
    yield pr, c, ofp
    pr.close()
    c.close()


def _verdicts(pr, ofp, pf):
    return pr.verify(pf), _oracle.plonk_verify_gates(pf, pr.cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST)


def test_the_combination_of_a_device_opening_proof_proves_and_verifies(ctx, opened, prover):
    import sipp_amd
    data, _, _ = opened
    pr, c, ofp = prover
    circ = pr.circ
    cs = circ.constants_sigmas()
    assert (pr.cap == _oracle.Batch(cs, circ.log_n, rate_bits=3, cap_height=4).cap).all()
    L = sipp_amd.lib()
    for round_, args in enumerate(data):                           # the second opening proof goes through the same circuit data
        pis = circ.public_inputs(*args)
        pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
        pw = circ.partial_witness(*args)
        want = rd.replay(pw, cs[:5], circ.generators(), pih, circ.schedule())
        if round_ == 0:                                            # the device witness (the generation CircuitData.prove runs) = the reading
            sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
            try:
                for route in (0, REDUCE_ONE_LANE):
                    assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
                    d_w = dev(pw)
                    ctx.plonk_generate_witness_levels(d_w, dev(cs[:5]), circ.log_n, circ.generators(), pih, sched)
                    assert first_mismatch(host(d_w), want) is None, route
            finally:
                assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
        pf = pr.prove(*args)
        ref = _oracle.plonk_prove_gates(want, cs, circ.log_n, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST, pis)
        assert len(pf) == len(ref) and (pf == ref).all(), round_
        assert _verdicts(pr, ofp, pf) == ((0, 0), 0)


@pytest.mark.parametrize("tamper", ["leaf_value", "opened_value", "point", "old"])
def test_tampered_inputs_are_refused_and_the_prover_goes_on(opened, prover, tamper):
    data, _, _ = opened
    pr, c, ofp = prover
    alpha, points, vals, queries = data[0]
    points, vals, queries = list(points), [list(v) for v in vals], [(x, list(lv), old) for x, lv, old in queries]
    bump = lambda p, l: tuple((v + (k == l)) % P for k, v in enumerate(p))
    if tamper == "leaf_value":
        queries[1][1][3] = (queries[1][1][3] + 1) % P
    elif tamper == "opened_value":
        vals[1][2] = bump(vals[1][2], 1)
    elif tamper == "point":
        points[0] = bump(points[0], 0)
    else:
        queries[2] = (queries[2][0], queries[2][1], bump(queries[2][2], 1))
    pf = pr.prove(alpha, points, vals, queries)
    (st, stage), orc = _verdicts(pr, ofp, pf)
    assert st != 0 and orc != 0, (st, stage, orc)
    good = pr.prove(*data[0])
    assert _verdicts(pr, ofp, good) == ((0, 0), 0)
