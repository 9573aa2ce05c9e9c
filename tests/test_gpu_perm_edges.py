"""The permutation argument on the device (plonk_chunk_kernel, plonk_scan_kernel, plonk_pp_kernel, the permutation terms of
plonk_quotient_kernel) on the catalogue of tests/_perm_cases.py: Z and the partial products word for word against the catalogue's
Python-integer expectation, quotient chunks and whole proofs word for word against oracle/plonk.c, whose verifier accepts the device's
proofs; the refusals by their exact codes, each followed by a good call on the same ctx.  No entry is skipped: what the device cannot
take is in a refusal list with its code."""
import ctypes as C

import numpy as np
import pytest

from tests import _oracle
from tests import _perm_cases as pc
from tests._device import dev, host
from tests.test_gpu_fri_generic import to_params

pytestmark = pytest.mark.gpu

P = pc.P
A = dict(pc.ENTRIES_A)
B = dict(pc.ENTRIES_B)


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def device_zs(ctx, e):
    import sipp_amd
    gp = sipp_amd.PlonkParams(e["R"], e["D"], e["C"])
    return host(ctx.plonk_zs(dev(e["wires"]), dev(e["sigmas"]), e["log_n"], gp, e["betas"], e["gammas"]))


def good_call(ctx):
    e = A["shape_n5_R9_D8_C2"]()
    msg = pc.first_mismatch(device_zs(ctx, e), e["zs"])
    assert msg is None, "after the refusal: " + msg


@pytest.mark.parametrize("name", pc.IDS_A)
def test_zs_and_partial_products_are_the_catalogues(ctx, name):
    """sipp_plonk_zs_partial_products, handed the entry's operands as they are (non-canonical ones included), against zs_exact"""
    e = A[name]()
    got = device_zs(ctx, e)
    assert got.shape == e["zs"].shape
    msg = pc.first_mismatch(got, e["zs"])
    assert msg is None, msg


@pytest.mark.parametrize("case", pc.REFUSALS_A, ids=[r[0] for r in pc.REFUSALS_A])
def test_zs_refusals(ctx, case):
    """check() refuses before any kernel runs (the buffers are those of a small shape it accepts); the ctx computes afterwards"""
    import sipp_amd
    _, log_n, R, D, Cn, code = case
    gp = sipp_amd.PlonkParams(R, D, Cn)
    w = dev(np.zeros((R, 32), dtype=np.uint64))
    out = dev(np.zeros((64, 32), dtype=np.uint64))
    ch = ctx._u64([3] * Cn)
    assert ctx.L.sipp_plonk_zs_partial_products(ctx.h, w.data_ptr(), w.data_ptr(), log_n, C.byref(gp), ch, ch, out.data_ptr()) == code
    assert (host(out) == 0).all()
    good_call(ctx)


def leaf_order(nat, log_n, log_d, rate_bits, fill):
    """[K][N D] natural order on the quotient coset -> [K][N << rate_bits] leaf order (the coset is the first N D leaves)"""
    nd = (1 << log_n) << log_d
    out = np.full((nat.shape[0], (1 << log_n) << rate_bits), fill, dtype=np.uint64)
    out[:, :nd] = nat[:, pc.bitrev_order(log_n + log_d)]
    return out


def reduced(v):
    return [x % P for x in v]


def quotient_pair(ctx, e, betas, gammas, alphas, gate_terms=None):
    """(device, oracle) quotient chunks: the device from its own committed LDEs and the raw challenges, the oracle from coefficients and
    the reduced ones; Z and the partial products compared on the way"""
    import sipp_amd
    log_n, rb = e["log_n"], e["rate_bits"]
    op, gp = _oracle.plonk_params(e["R"], e["D"], e["C"]), sipp_amd.PlonkParams(e["R"], e["D"], e["C"])
    d_w, d_s = dev(e["wires"]), dev(e["sigmas"])
    ref_zs = _oracle.plonk_zs(e["wires"], e["sigmas"], log_n, op, reduced(betas), reduced(gammas))
    got_zs = ctx.plonk_zs(d_w, d_s, log_n, gp, betas, gammas)
    msg = pc.first_mismatch(host(got_zs), ref_zs)
    assert msg is None, "zs: " + msg
    _, _, (wc, wl, _) = ctx.commit_ex(d_w, log_n, rb, 1)
    _, _, (sc, sl, _) = ctx.commit_ex(d_s, log_n, rb, 1)
    _, _, (zc, zl, _) = ctx.commit_ex(got_zs, log_n, rb, 1)
    if gate_terms is None:
        ref = _oracle.plonk_quotient_chunks(host(wc), host(sc), host(zc), log_n, op, reduced(betas), reduced(gammas), reduced(alphas))
        got = ctx.plonk_quotient_chunks(wl, sl, zl, log_n, rb, gp, betas, gammas, alphas)
    else:
        log_d = e["D"].bit_length() - 1
        nat = _oracle.plonk_gate_terms_coset(host(wc), log_n, log_d, gate_terms)
        lifted = pc.lift(nat)
        assert (lifted >= np.uint64(P)).any() and (lifted.astype(object) % P == nat.astype(object)).all()
        ref = _oracle.plonk_quotient_chunks_ex(host(wc), host(sc), host(zc), log_n, op, reduced(betas), reduced(gammas), reduced(alphas), nat)
        d_gt = dev(leaf_order(lifted, log_n, log_d, rb, 0xDEADBEEF))      # rows outside the quotient coset are never read
        got = ctx.plonk_quotient_chunks_ex(wl, sl, zl, log_n, rb, gp, betas, gammas, alphas, d_gt)
    return host(got), ref


@pytest.mark.parametrize("name", pc.IDS_B)
def test_quotient_chunks_and_whole_proofs_are_the_oracles(ctx, name):
    import sipp_amd
    e = B[name]()
    log_n, Cn = e["log_n"], e["C"]
    if e["kind"] == "proof":
        rng = np.random.default_rng(3)
        betas, gammas, alphas = ([int(v) for v in _oracle.rand_field(rng, (Cn,))] for _ in range(3))
    else:
        betas, gammas, alphas = e["betas"], e["gammas"], e["alphas"]
    got, ref = quotient_pair(ctx, e, betas, gammas, alphas, e.get("num_mul"))
    msg = pc.first_mismatch(got, ref)
    assert msg is None, "quotient chunks: " + msg
    if e["zero_quotient"]:
        assert (got == 0).all()
    if e["kind"] != "proof":
        return
    op, gp = _oracle.plonk_params(e["R"], e["D"], Cn), sipp_amd.PlonkParams(e["R"], e["D"], Cn)
    fp = pc.fri_params(e)
    ref_pf = _oracle.plonk_perm_prove(e["wires"], e["sigmas"], log_n, op, fp, digest=pc.DIGEST)
    pf = ctx.plonk_perm_prove(dev(e["wires"]), dev(e["sigmas"]), log_n, gp, to_params(fp), digest=pc.DIGEST)
    assert len(pf) == len(ref_pf)
    diff = np.nonzero(pf != ref_pf)[0]
    assert diff.size == 0, "first mismatch at word %d of %d" % (diff[0], len(ref_pf))
    cap = _oracle.Batch(e["sigmas"], log_n, rate_bits=e["rate_bits"], cap_height=pc.FRI["cap_height"]).cap
    assert _oracle.plonk_perm_verify(pf, cap, op, fp, digest=pc.DIGEST) == 0


@pytest.mark.parametrize("case", pc.REFUSALS_B, ids=[r[0] for r in pc.REFUSALS_B])
def test_quotient_refusals(ctx, case):
    """the quotient's own limits by their exact codes; D = 16 is refused here although sipp_plonk_zs_partial_products computes with it"""
    import sipp_amd
    name, R, D, Cn, rb, (n_gt, _), code = case
    log_n = 10
    gp = sipp_amd.PlonkParams(R, D, Cn)
    cols = dev(np.zeros((max(R, Cn * pc.num_chunks(R, D)), (1 << log_n) << min(rb, 3)), dtype=np.uint64))
    out = dev(np.zeros((Cn * D, 1 << log_n), dtype=np.uint64))
    one = ctx._u64([1] * Cn)
    rc = ctx.L.sipp_plonk_quotient_chunks_ex(ctx.h, cols.data_ptr(), cols.data_ptr(), cols.data_ptr(), log_n, rb, C.byref(gp), one, one, one, None,
                                             n_gt, out.data_ptr())
    assert rc == code and (host(out) == 0).all()
    if name == "chunk_size_16_rate_3":
        rng = np.random.default_rng(9)
        w, s = _oracle.rand_field(rng, (R, 32)), _oracle.rand_field(rng, (R, 32))
        e = dict(log_n=5, R=R, D=D, C=Cn, wires=w, sigmas=s, betas=[5], gammas=[6])
        msg = pc.first_mismatch(device_zs(ctx, e), pc.zs_exact(w, s, 5, D, [5], [6])[0])
        assert msg is None, msg
    good_call(ctx)
