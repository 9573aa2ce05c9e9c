"""The u32 and nonnative generators (kinds 19 - 21, include/sipp_hip.h) and the transcript circuit on the device.  The catalogue of
tests/_transcript_cases.py, one case per row, against its Python-integer reading cell for cell -- the refused rows' zeros included --
through the row-local entry, a level of 16384 rows (one lane per row) and every sixteen-lane kernel's U32 instantiation; the refusal of
a layout that leaves the wire table; then SippTranscriptCircuit at n = 4 and n = 8: the device witness against the replay, the proof
against the oracle's for that witness, both verifiers, prove_words against prove, check_obligations."""
import numpy as np
import pytest

from tests import _transcript_cases as tc
from tests import _witness_reading as rd
from tests._device import NO_GRAPH, dev, first_mismatch, host, levels

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 28)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide():
    return tc.catalogue_table(15)


@gpu
def test_catalogue_row_local(ctx, wide):
    w, k, gens, want, _ = wide
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, dev(k), 15, gens)
    ctx.sync()
    assert first_mismatch(host(d_w), want) is None
    for name in tc.REFUSED:                                     # the refused rows' 24 zeros are part of the comparison
        r = sorted(tc.CATALOGUE).index(name)
        assert not want[16:40, r].any() and w[16:40, r].all()


@gpu
@pytest.mark.parametrize("route", [0, NO_GRAPH], ids=["graph", "launches"])
def test_catalogue_on_a_level_of_16384_rows_and_one_of_16383(ctx, wide, route):
    """level 0 = rows 0 .. 16382 (sixteen lanes per row, the row on lane 0 of plonk_witness_level_coop_kernel<true>), level 1 = rows
    16384 .. 32767 (one lane per row); row 16383 is in no level and stays as it was"""
    import sipp_amd
    w, k, gens, want, _ = wide
    want = want.copy()
    want[:, 16383] = w[:, 16383]
    sc = levels([np.arange(16383), np.arange(16384, 32768)])
    L = sipp_amd.lib()
    try:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
        d_w = dev(w)
        ctx.plonk_generate_witness_levels(d_w, dev(k), 15, gens, None, sipp_amd.PlonkSchedule.from_dict(sc))
        assert first_mismatch(host(d_w), want) is None
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


# generator lists that pick each sixteen-lane kernel (tests/test_gpu_poseidon_mds_generator.py): row 60 holds the Poseidon-family
# generator (selector value 5), no row holds the others.  The Poseidon layouts stay clear of the catalogue rows' cells: none is held.
POSEIDON = (rd.GEN_POSEIDON, 0, 5, 0, 12, 24, 0, 0)
SWAP = (rd.GEN_POSEIDON_SWAP, 0, 5, 0, 12, 29, 24, 25)
THIN = {"coop": [POSEIDON], "coop_rows": [SWAP], "coop_rows_interp": [SWAP, (rd.GEN_COSET_INTERPOLATION, 0, 6, 4, 7, 7, 0, 0)],
        "coop_rows_reduce": [SWAP, (rd.GEN_REDUCING_EXT, 0, 7, 19, 7, 0, 0, 0)]}


@gpu
@pytest.mark.parametrize("kernel", sorted(THIN))
def test_catalogue_on_thin_levels_beside_a_poseidon_row(ctx, kernel):
    """every case once, in levels of 1, 5 and the rest of the rows: each row runs on lane 0 of its sixteen"""
    import sipp_amd
    w, k, gens, _, names = tc.catalogue_table(10, seed=1902, repeat=False)
    n_cases = len(names)
    assert n_cases == len(tc.CATALOGUE) < 60
    k[0, 60] = 5
    w[:25, 60] = np.random.default_rng(1903).integers(0, tc.P, 25, dtype=np.uint64)
    w[24, 60] = 1                                               # the swap wire
    gens = gens + THIN[kernel]
    sc = levels([[3], [10, 11, 60, 13, 14], [r for r in range(n_cases) if r not in (3, 10, 11, 13, 14)]])
    want = rd.replay(w, k, gens, None, sc)
    assert (want[12:24, 60] != w[12:24, 60]).all() and (want[:, n_cases:60] == w[:, n_cases:60]).all()
    d_w = dev(w)
    ctx.plonk_generate_witness_levels(d_w, dev(k), 10, gens, None, sipp_amd.PlonkSchedule.from_dict(sc))
    assert first_mismatch(host(d_w), want) is None


# p0 .. p3 on a table of 135 wires
BAD_LAYOUTS = {"arith_past_the_table": (tc.GEN_U32_ARITHMETIC, 4, 38, 16, 0), "arith_stride_short": (tc.GEN_U32_ARITHMETIC, 1, 37, 16, 0),
               "arith_17_limbs": (tc.GEN_U32_ARITHMETIC, 1, 40, 17, 0), "add_past_the_table": (tc.GEN_U32_ADD_MANY, 4, 38, 16, 3),
               "add_no_addend": (tc.GEN_U32_ADD_MANY, 1, 38, 0, 3), "add_stride_short": (tc.GEN_U32_ADD_MANY, 1, 37, 16, 3),
               "nonnative_op_2": (tc.GEN_NONNATIVE, 2, 0, 8, 16), "nonnative_out_past_the_table": (tc.GEN_NONNATIVE, 0, 0, 8, 112),
               "nonnative_out_meets_x": (tc.GEN_NONNATIVE, 0, 23, 40, 0), "nonnative_out_meets_m": (tc.GEN_NONNATIVE, 1, 40, 23, 0),
               "nonnative_x_wraps_32_bits": (tc.GEN_NONNATIVE, 0, 0xFFFFFFFC, 8, 16)}


@gpu
@pytest.mark.parametrize("name", sorted(BAD_LAYOUTS))
def test_a_layout_outside_the_table_is_badarg_and_the_next_call_is_served(ctx, name):
    import sipp_amd
    w, k, gens, want, _ = tc.catalogue_table(10, seed=1904)
    kind, p = BAD_LAYOUTS[name][0], BAD_LAYOUTS[name][1:]
    bad = [(kind, 0, 9) + p + (0,)]
    sched = sipp_amd.PlonkSchedule.from_dict(levels([np.arange(1024)]))
    d_w, d_k = dev(w), dev(k)
    for call in (lambda g: ctx.plonk_generate_witness(d_w, d_k, 10, g), lambda g: ctx.plonk_generate_witness_levels(d_w, d_k, 10, g, None, sched)):
        with pytest.raises(sipp_amd.SippError) as e:
            call(gens + bad)
        assert e.value.code == -1                               # SIPP_E_BADARG
        ctx.sync()
        assert first_mismatch(host(d_w), w) is None
        call(gens)
        ctx.sync()
        assert first_mismatch(host(d_w), want) is None
        d_w.copy_(dev(w))


# ---- the transcript circuit -----------------------------------------------------------------------------------------------------------------
DIGEST = (61, 62, 63, 64)


@pytest.fixture(scope="module", params=[4, 8], ids=["n4", "n8"])
def prover(request):
    import ctypes as C

    import sipp_amd
    from sipp_amd import transcript as tr
    from tests.test_gpu_fri_generic import to_params
    from tests.test_oracle_plonk import fri
    n = request.param
    circ = tr.SippTranscriptCircuit(n)
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    c = sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc)))
    pr = tr.SippTranscriptProver(c, n, fri=gfp, digest=DIGEST)
    yield pr, ofp, tc.fixture(n)
    pr.close()
    c.close()


@gpu
def test_the_transcript_circuit_end_to_end(ctx, prover):
    """the device witness equals the replay cell for cell; the proof is word for word the oracle's for that witness; both verifiers
    accept it; prove_words gives prove's bytes; check_obligations holds for the fixture's records and fails after one exponent limb"""
    import sipp_amd
    from tests import _oracle
    pr, ofp, (st, rw, ex, d) = prover
    c = pr.circ
    ch = pr.challenges_of(d["fq12"])
    assert ch == [v for x, xi in ex for v in tc.limbs(x) + tc.limbs(xi)]
    cs = c.constants_sigmas()
    pis = c.public_inputs(st, rw, ch)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    pw = c.partial_witness(st, rw, ch)
    want = rd.replay(pw, cs[:c.num_constants], c.generators(), pih, c.schedule())
    d_w = dev(pw)
    ctx.plonk_generate_witness_levels(d_w, dev(cs[:c.num_constants]), c.log_n, c.generators(), pih, sipp_amd.PlonkSchedule.from_dict(c.schedule()))
    assert first_mismatch(host(d_w), want) is None
    for k in range(c.rounds):
        assert tc.value([int(want[w, r]) for w, r in c.x_cells[k]]) == ex[k][0]
        assert tc.value([int(want[w, r]) for w, r in c.xinv_cells[k]]) == ex[k][1]
    op = _oracle.plonk_params(80, 8, 2)
    pf = pr.prove(st, rw, ch)
    ref = _oracle.plonk_prove_gates(want, cs, c.log_n, op, ofp, pr.circuit, DIGEST, pis)
    assert len(pf) == len(ref) and (pf == ref).all()
    assert pr.verify(pf) == (0, 0) and _oracle.plonk_verify_gates(pf, pr.cap, op, ofp, pr.circuit, DIGEST) == 0
    again = pr.prove_words(st, rw, ch)
    assert len(again) == len(pf) and (again == pf).all()
    assert pr.check_obligations(pis, d["g1"], d["g2"], d["fq12"])
    for name, at in (("g1", 33), ("g2", 64), ("fq12", 199)):
        recs = {k: d[k].copy() for k in ("g1", "g2", "fq12")}
        recs[name][0, at] ^= 1
        assert not pr.check_obligations(pis, recs["g1"], recs["g2"], recs["fq12"])
    # a claimed x limb that is not the transcript's: the proof is refused by both verifiers, and the prover goes on
    bad = list(ch)
    bad[2] ^= 1
    pf_bad = pr.prove(st, rw, bad)
    assert pr.verify(pf_bad)[0] != 0 and _oracle.plonk_verify_gates(pf_bad, pr.cap, op, ofp, pr.circuit, DIGEST) != 0
    assert (pr.prove(st, rw, ch) == pf).all()


@gpu
def test_a_generator_outside_the_wire_table_is_badarg_and_the_ctx_proves_afterwards(prover):
    """the circuit's own generators with the nonnative outputs moved past the last wire, on the prover's ctx: SIPP_E_BADARG, the table
    untouched; the same ctx then proves"""
    import sipp_amd
    pr, ofp, (st, rw, ex, d) = prover
    c, pctx = pr.circ, pr.data.ctx
    ch = pr.challenges_of(d["fq12"])
    gens = [g if g[0] != tc.GEN_NONNATIVE else g[:6] + (c.num_wires - 23,) + g[7:] for g in c.generators()]
    assert gens != c.generators()
    pw = c.partial_witness(st, rw, ch)
    d_w = dev(pw)
    with pytest.raises(sipp_amd.SippError) as e:
        pctx.plonk_generate_witness_levels(d_w, dev(c.constants_sigmas()[:c.num_constants]), c.log_n, gens, [1, 2, 3, 4],
                                           sipp_amd.PlonkSchedule.from_dict(c.schedule()))
    assert e.value.code == -1                                   # SIPP_E_BADARG
    pctx.sync()
    assert first_mismatch(host(d_w), pw) is None
    assert pr.verify(pr.prove(st, rw, ch)) == (0, 0)
