"""The exponentiation traces on the GPU (sipp_amd/csrc/trace.hip and the lookup columns built from them) against the CPU oracle over the
edge catalogue tests/_exp_edges.py, which tests/test_oracle_exp_edges.py pins to Python integers: outputs, traces cell for cell in both
table variants, whole proofs word for word at the smallest shapes (the permuted lookup columns and Z are visible only there), and
refusals (SIPP_E_WITNESS, -8) for exactly the AIR variants the catalogue names."""
import functools

import numpy as np
import pytest

from tests import _exp_edges as E
from tests import _oracle, _verify

pytestmark = pytest.mark.gpu
KINDS = [0, 4, 1, 5, 2]


def arr(kind, recs, blank=False):
    return np.array(E.words(kind, recs, blank), dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    L = sipp_amd.lib()
    need = max(L.sipp_workspace_bytes(k, n) for k, n in [(k, 32) for k in KINDS] + [(4, 128), (5, 128)])
    c = sipp_amd.Ctx(workspace_bytes=need)
    yield c
    c.close()


def assert_same_cells(got, want, what):
    assert got.shape == want.shape, what
    if not (got == want).all():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d cells differ; first (col,row): %s" % (what, len(bad), bad[:8].tolist()))


def pick(kind, prefix, e=None):
    return next(r for r in E.records(kind) if r.name.startswith(prefix) and (e is None or r.e == e))


@functools.lru_cache(None)
def proof_batch(kind):
    """the smallest batches whose whole proofs are compared: G1: the point next to x = p - 1 (e = 2^255 + 1), the point next to TOP
    (e = 2^256 - 1) and the last-limb pair in both orders; G2: half of the same recipe; Fq12: the zero record"""
    k = E.base_kind(kind)
    if k == 0:
        return arr(0, [pick(0, "near_pm1__", (1 << 255) + 1), pick(0, "near_top__", (1 << 256) - 1), pick(0, "limb15_pos_e3"), pick(0, "limb15_neg_e3")])
    if k == 1:
        return arr(1, [pick(1, "near_top__", (1 << 256) - 1), pick(1, "limb31_neg_e3")])
    return arr(2, [pick(2, "zero_zero_0")])


@functools.lru_cache(None)
def oracle_proof(kind):
    return _oracle.stark_prove(kind, proof_batch(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_outputs_match_the_python_integers(ctx, kind):
    """sipp_exp_outputs (curve_outputs_kernel, the outputs-only Fq12 chain) on records whose output words are blank"""
    recs = E.records(kind)
    got = ctx.exp_outputs(kind, arr(kind, recs, blank=True))
    want = arr(kind, recs)
    bad = [recs[i].name for i in np.flatnonzero((got != want).any(axis=1))]
    assert not bad, "kind %d: outputs differ for %s" % (kind, bad[:6])


@pytest.mark.parametrize("kind", KINDS)
def test_trace_matches_the_oracle_cell_for_cell_u8(ctx, kind):
    from sipp_amd._lib import to_host
    ios = arr(kind, E.records(kind))
    ref = _oracle.Trace(kind, ios)
    assert ref.air.table_bits == 8 and 13 <= ref.log_n <= 15
    assert ctx.shape(kind, ios.shape[0])[:2] == (ref.log_n, ref.width)
    got = to_host(ctx.trace_build(kind, ios))
    assert_same_cells(got, ref.array(), "kind %d" % kind)


@pytest.mark.parametrize("kind", [4, 5])
def test_hardened_trace_matches_the_oracle_cell_for_cell_u16(ctx, kind):
    """the catalogue tiled to 128 records: N = 2^16, the u16-table variant (one checked cell per limb)"""
    from sipp_amd._lib import to_host
    recs = E.records(kind)
    ios = arr(kind, [recs[i % len(recs)] for i in range(128)])
    ref = _oracle.Trace(kind, ios)
    assert ref.air.table_bits == 16 and ref.log_n == 16 and ref.air.hardened == 1
    got = to_host(ctx.trace_build(kind, ios))
    try:
        assert_same_cells(got, ref.array(), "kind %d (u16)" % kind)
    finally:
        del got, ref


@pytest.mark.parametrize("kind", KINDS)
def test_proof_matches_the_oracle_word_for_word(ctx, kind):
    ios = proof_batch(kind)
    want = oracle_proof(kind)
    pf = ctx.prove(kind, ios)
    assert int(pf[1]) == kind and pf.shape == want.shape and (pf == want).all()
    assert _verify.both_accept(pf)


def test_fq12_proof_of_maximal_coefficients_and_exponent(ctx):
    """x = offset = all twelve coefficients p - 1, e = 2^256 - 1: one record"""
    ios = arr(2, [pick(2, "pm1_pm1_max")])
    pf = ctx.prove(2, ios)
    want = _oracle.stark_prove(2, ios)
    assert pf.shape == want.shape and (pf == want).all()
    assert _verify.both_accept(pf)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_refusal_parity(ctx, kind):
    """every `refused` record between valid ones: prove and trace_build return SIPP_E_WITNESS for the variants the catalogue names; the other
    variant builds the oracle's trace and a proof both verifiers accept; after each refusal the ctx proves a valid batch as before"""
    import sipp_amd
    from sipp_amd._lib import to_host
    good = E.records(kind)
    for ref in E.refused(kind):
        ios = arr(kind, [good[0], ref, good[1], good[2]])
        for k, no_witness in ((kind, ref.plain),) + (((kind + 4, ref.hardened),) if kind < 2 else ()):
            if no_witness:
                for call in (ctx.prove, ctx.trace_build):
                    with pytest.raises(sipp_amd.SippError) as e:
                        call(k, ios)
                    assert e.value.code == -8, (ref.name, k, call.__name__)
                with pytest.raises(RuntimeError):
                    _oracle.Trace(k, ios)
                assert (ctx.prove(k, proof_batch(k)) == oracle_proof(k)).all(), (ref.name, k)
            else:
                want = _oracle.Trace(k, ios)
                assert_same_cells(to_host(ctx.trace_build(k, ios)), want.array(), "%s kind %d" % (ref.name, k))
                pf = ctx.prove(k, ios)
                assert int(pf[1]) == k and _verify.both_accept(pf), (ref.name, k)
                assert (pf[-4 * ios.shape[1]:].reshape(4, -1) == ios).all()
