"""The two host drivers under every proof and under the native chain (sipp_amd/csrc/trace.hip: sipp_trace_fill fills a main trace,
sipp_outputs_fill writes the output words into the records) through the public API only: what the outputs path refuses and what it never
reads, both drivers in alternation on ONE ctx for all seven kinds (the row scratch, the lookup scratch and the cached tables of one must
not leak into the other), proofs and the native chain's later fold round (sipp_fold_outputs) behind them, and the event brackets each
call records -- scripts and bench.py's per-kernel breakdown read those names."""
import numpy as np
import pytest

from tests import _exp_edges as E
from tests import _oracle
from tests import _pairing_cases as PC
from tests import test_gpu_exp_edges as X          # its proof batches and the oracle's proofs of them (computed once per session)
from tests.test_gpu_mapg2 import messages

pytestmark = pytest.mark.gpu
WITNESS = -8
# what curve_outputs_kernel refuses: an x or an offset off the curve, an output at infinity
ALWAYS_REFUSED = {"x_off_curve", "offset_off_curve", "output_identity_e5", "output_identity_e1"}


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    L = sipp_amd.lib()
    c = sipp_amd.Ctx(workspace_bytes=max(L.sipp_workspace_bytes(k, n) for k, n in [(0, 4), (4, 4), (1, 4), (5, 4), (2, 4), (3, 2), (6, 1)]))
    yield c
    c.close()


_cache = {}


def batch(kind):
    """(records with blank output words, complete records, the oracle's trace) of a small valid batch of the kind, computed once"""
    if kind not in _cache:
        if kind == 3:
            _, words = messages(2)
            blank = np.zeros((2, 48), dtype=np.uint32)
            blank[:, :16] = words
            full = _oracle.map_to_g2(words)
        elif kind == 6:
            from oracle.py import bn254 as bn
            blank = np.zeros((1, 144), dtype=np.uint32)
            blank[0, :48] = bn.g1_to_u32(bn.G1) + bn.g2_to_u32(bn.G2)
            full = blank.copy()
            full[0, 48:] = _oracle.pairing(blank[0, :48])
        else:
            recs = E.records(kind)[:4]
            blank, full = X.arr(kind, recs, blank=True), X.arr(kind, recs)
        ref = _oracle.Trace(kind, full)             # (array() is a view of memory the Trace frees: copy while it is alive)
        _cache[kind] = (blank, full, ref.array().copy())
        del ref
    return _cache[kind]


def assert_both_drivers(ctx, kind, what):
    from sipp_amd._lib import to_host
    blank, full, trace = batch(kind)
    assert (ctx.exp_outputs(kind, blank) == full).all(), "%s: outputs of kind %d" % (what, kind)
    X.assert_same_cells(to_host(ctx.trace_build(kind, full)), trace, "%s: trace of kind %d" % (what, kind))


# ---------------- 1. what the outputs path refuses ----------------
@pytest.mark.parametrize("kind", [0, 1])
def test_outputs_refusals_of_the_curves(ctx, kind):
    """every `refused` record of the catalogue between two valid ones, output words blank (3 records, 2^11 rows): points off the curve and
    outputs at infinity are refused (-8); a wrong CLAIMED output is not -- the outputs path never reads the claimed words; every other
    record is refused or yields its Python-integer output, nothing else; after a refusal the ctx works as before"""
    import sipp_amd
    good = E.records(kind)
    for r in E.refused(kind):
        # (the catalogue's `out` is the CLAIMED output: the true one where a variant proves the record, a flipped bit for wrong_output)
        true = r._replace(out=E.g_out(kind, r.x, r.off, r.e)) if r.name == "wrong_output" else r
        ios, want = X.arr(kind, [good[0], r, good[1]], blank=True), X.arr(kind, [good[0], true, good[1]])
        try:
            got = ctx.exp_outputs(kind, ios)
        except sipp_amd.SippError as e:
            print("kind %d %s: refused (%d)" % (kind, r.name, e.code))
            assert e.code == WITNESS and r.name != "wrong_output", (kind, r.name, e.code)
            assert_both_drivers(ctx, kind, "after the refusal of %s" % r.name)
            continue
        print("kind %d %s: outputs returned" % (kind, r.name))
        assert r.name not in ALWAYS_REFUSED, (kind, r.name)
        assert (got == want).all(), (kind, r.name)


# ---------------- 2. both drivers in alternation on one ctx ----------------
@pytest.mark.parametrize("kind", [0, 4, 1, 5, 2, 3, 6])
def test_outputs_trace_outputs_on_one_ctx(ctx, kind):
    blank, full, _ = batch(kind)
    assert_both_drivers(ctx, kind, "alternation")
    assert (ctx.exp_outputs(kind, blank) == full).all()
    if kind <= 2:
        pf = ctx.prove(kind, X.proof_batch(kind))
        want = X.oracle_proof(kind)
        assert pf.shape == want.shape and (pf == want).all()


def test_native_chain_between_proofs_on_the_same_ctx(ctx):
    """sipp_verify_native at n = 4: its later round folds through sipp_fold_outputs (two chains on two streams, two row blocks); the ctx
    then proves the G1 batch word for word as before"""
    A, B, honest = PC.fixture(4)
    d = np.load("tests/golden/sipp_n4_ios.npz")
    assert_both_drivers(ctx, 0, "before the native chain")
    ok, st, ios = ctx.verify_native(A, B, honest)
    assert ok and (st == d["statement"]).all()
    for got, key in zip(ios, ("g1", "g2", "fq12")):
        assert got.shape == d[key].shape and (got == d[key]).all(), key
    pf = ctx.prove(0, X.proof_batch(0))
    assert (pf == X.oracle_proof(0)).all()
    assert_both_drivers(ctx, 1, "after the native chain")


# ---------------- 3. the event brackets ----------------
def brackets(ctx, call):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        call()
        rep = ctx.profile_report()
    finally:
        ctx.profile(False)
    return {k: v["calls"] for k, v in rep.items() if k.startswith(("trace_", "lookup_", "mapg2_"))}


TRACE_BRACKETS = ["trace_curve_chain", "trace_curve_rows", "trace_check_outputs", "trace_exp_table", "trace_gadgets", "lookup_hist", "lookup_scan",
                  "lookup_fill"]


@pytest.mark.parametrize("kind,names", [(0, TRACE_BRACKETS), (4, TRACE_BRACKETS + ["trace_harden"])])
def test_brackets_of_one_trace_build(ctx, kind, names):
    assert brackets(ctx, lambda: ctx.trace_build(kind, batch(kind)[1])) == {k: 1 for k in names}


@pytest.mark.parametrize("kind,name", [(0, "trace_curve_chain"), (1, "trace_curve_chain"), (2, "trace_fq12_chain"), (3, "mapg2_outputs"), (6, "trace_pairing")])
def test_brackets_of_one_exp_outputs(ctx, kind, name):
    assert brackets(ctx, lambda: ctx.exp_outputs(kind, batch(kind)[0])) == {name: 1}
