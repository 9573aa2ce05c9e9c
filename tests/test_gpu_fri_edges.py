"""Generic opening proofs (sipp_commit_batch_ex + sipp_fri_prove_openings) at the edges of their documented range: every case of
tests/_fri_cases.py is committed and proved on the device and held against oracle/fri.c -- every cap, the proof word for word, the
challenger afterwards -- and the device's proof goes through the oracle's verifier and the library's.  The cases reach what random
data at 2^10 .. 2^13 never does: the point zero (a shift instead of a division), points with a zero component and z^n = -1, structured
and all-zero columns, no reduction round, cap heights 0 and 8, a layer of exactly 2^cap_height leaves, 1 and 1024 queries, eight
oracles with leaves on both sides of hash_or_noop's 4 words, empty ranges and batches without a polynomial, a challenger with pending
input / output, the proof-of-work search beyond its first launch, sipp_k_openings in segments that do not divide n, the multi-chunk
tile carry of the division at 2^19.  Where a case is about a route, the profile's call counts name the route, so that a routing change
cannot silently retarget it.  Nothing here has a tolerance: field arithmetic, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _fri_cases as fc
from tests import _oracle, _verify
from tests.test_gpu_fri_generic import gpu_challenger, to_params

pytestmark = pytest.mark.gpu
P = fc.P
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=2 << 30)
    yield c
    c.close()


def commit(ctx, inst):
    """the case's oracles on the device, each cap equal to the oracle's; returns the Oracle structs and the tensors behind them"""
    from sipp_amd._lib import to_device
    devs, keep = [], []
    for k, (data, from_coeffs, salt) in enumerate(fc.device_inputs(inst)):
        od, cap, bufs = ctx.commit_ex(to_device(data), inst.log_n, inst.fp.rate_bits, inst.fp.cap_height, from_coeffs=from_coeffs,
                                      salt=None if salt is None else to_device(salt))
        assert (cap == inst.oracles[k].cap).all(), "cap of oracle %d" % k
        devs.append(od)
        keep.append(bufs)
    return devs, keep


def prove_and_compare(ctx, inst, devs, och):
    """what test_generic_opening_proof_identical_to_oracle asserts, for a transcript that starts at `och`; returns (proof, profile)"""
    import sipp_amd
    before = bytes(och)
    gch = sipp_amd.Challenger.from_buffer_copy(before)
    ref = _oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, och)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        got = ctx.fri_prove_openings(devs, inst.batches, inst.log_n, to_params(inst.fp), gch)
        rep = ctx.profile_report()
    finally:
        ctx.profile(False)
    assert len(got) == len(ref), (len(got), len(ref))
    diff = np.nonzero(got != ref)[0]
    assert diff.size == 0, "first mismatch at word %d of %d" % (diff[0], len(ref))
    assert bytes(gch) == bytes(och)             # state, pending input and unread output: the transcript continues identically
    start = lambda: _oracle.OrcChallenger.from_buffer_copy(before)
    assert _oracle.fri_verify_openings(got, *inst.verifier_args(), start()) == 0
    stage, _ = _verify.lib_fri_verify(got, *inst.verifier_args(), start())
    assert stage == 0                           # the library's own verifier (sipp_fri_verify_openings)
    return got, rep


def openings_segments(ncols, n):
    """sipp_k_openings: about 2048 blocks whatever the column count, at most 64 segments, a segment of at least 1024 rows"""
    return min(64, -(-2048 // ncols), n // 1024)


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_edge_case_proof_identical_to_oracle(ctx, case):
    inst = fc.build(case)
    n = 1 << inst.log_n
    devs, keep = commit(ctx, inst)
    got, rep = prove_and_compare(ctx, inst, devs, fc.challenger(case))
    calls = lambda name: rep[name]["calls"] if name in rep else 0
    zero_batches = sum(1 for pt, _ in inst.batches if pt == (0, 0))
    assert calls("fri_shift_down") == zero_batches and calls("fri_divide") == len(inst.batches) - zero_batches, sorted(rep)
    assert calls("fri_fold") == inst.fp.n_rounds
    if case.id.startswith("pow-"):
        assert (calls("pow_grind") == 0) == (inst.fp.pow_bits == 0)
        if inst.fp.pow_bits == 0:
            assert got[inst.witness_index()] == 0
    if case.id.startswith("wide_ragged"):
        for _, ranges in inst.batches:
            for _, b, e in ranges:
                segs = openings_segments(e - b, n)
                assert segs > 1 and n % segs != 0 and -(-n // segs) % 256 != 0, (b, e, segs)      # ragged segments, an idle part in the last trip
    if case.id == "long":
        assert n // 1024 > 256                  # more tile totals than one chunk of fri_divide_carry scans
    if case.id == "queries-1024":
        assert got[3] == 1024


@pytest.mark.parametrize("rule", [0, 1])
def test_pow_search_beyond_its_first_launch(ctx, rule):
    """sipp_k_pow_search grinds ascending batches of 2^max(12, pow_bits + 1) nonces and keeps the smallest witness of the first batch
    that holds one.  At 11 bits a launch covers 2^12 nonces: prefix seeds whose smallest witness (by the oracle) lies in launch 0, in
    launch 1 and in a later launch must each take exactly that many launches and return that witness."""
    found = fc.pow_scan(rule)
    assert sorted(found) == [0, 1, 2], "a launch class without a prefix seed: %r" % found
    inst = fc.build(fc.pow_case(rule, 0))
    assert inst.fp.pow_bits == fc.POW_SCAN_BITS and max(12, inst.fp.pow_bits + 1) == fc.POW_LAUNCH_BITS
    devs, keep = commit(ctx, inst)
    for cls, (s, w) in sorted(found.items()):
        launch = w >> fc.POW_LAUNCH_BITS
        assert (launch == cls) if cls < 2 else (launch >= 2)
        got, rep = prove_and_compare(ctx, inst, devs, _oracle.challenger([s, 1, 2]))
        assert got[inst.witness_index()] == w, (s, w)
        assert rep["pow_grind"]["calls"] == launch + 1, (s, w, rep["pow_grind"])


def raw_prove(ctx, devs, batches, log_n, params, gch):
    """sipp_fri_prove_openings itself: (status, the caller's proof buffer, filled with a sentinel before the call)"""
    import sipp_amd
    from sipp_amd._lib import FriBatch, Oracle, PolyRange
    L = sipp_amd.lib()
    oa = (Oracle * len(devs))(*devs)
    ba = (FriBatch * len(batches))()
    keep = []
    for i, (pt, ranges) in enumerate(batches):
        r = (PolyRange * len(ranges))(*[PolyRange(*x) for x in ranges])
        keep.append(r)
        ba[i].point[0], ba[i].point[1] = int(pt[0]), int(pt[1])
        ba[i].n_ranges = len(ranges)
        ba[i].ranges = r
    out = np.full(1 << 16, SENTINEL, dtype=np.uint64)
    n = C.c_size_t()
    rc = L.sipp_fri_prove_openings(ctx.h, oa, len(devs), ba, len(batches), log_n, C.byref(params), C.byref(gch), out.ctypes.data, len(out),
                                   C.byref(n))
    return rc, out


def test_refusals_leave_the_ctx_usable(ctx):
    case = fc.Case("refusals", widths=(3, 2), seed=5)
    inst = fc.build(case)
    devs, keep = commit(ctx, inst)
    good = to_params(inst.fp)
    all_cols = inst.batches[0][1]

    def refused(want, batches=None, log_n=10, params=good, n_in=None):
        gch, _ = gpu_challenger([7, 7, 7])
        if n_in is not None:
            gch.n_in = n_in
        before = bytes(gch)
        rc, out = raw_prove(ctx, devs, batches or inst.batches, log_n, params, gch)
        assert rc == want, (rc, want)
        assert (out == SENTINEL).all()              # refused before any proof word is written
        assert bytes(gch) == before                 # and the caller's transcript has not moved

    def params_with(arities, cap_height=None):
        p = to_params(inst.fp)
        p.n_rounds = len(arities)
        for i, a in enumerate(arities):
            p.arity_bits[i] = a
        if cap_height is not None:
            p.cap_height = cap_height
        return p
    # opening points in the trace subgroup: SIPP_E_SUBGROUP
    for z in (1, fc.root_of_unity(10), P - 1):
        refused(-5, batches=[((z, 0), all_cols)])
        refused(-5, batches=[inst.batches[0], ((z, 0), all_cols)])          # in a later batch as well
    # degree bits outside 10 .. 24: SIPP_E_UNSUPPORTED (only the parameter is that large: the refusal comes before anything is touched)
    refused(-7, log_n=9, params=params_with([4]))
    refused(-7, log_n=25, params=params_with([4, 4, 4, 4, 4]))
    # a round that would leave a layer with fewer leaves than its cap: the protocol forbids it, SIPP_E_BADARG
    refused(-1, params=params_with([4], cap_height=8))
    # a committed layer of fewer than 16 values (the third round would commit 2^3): SIPP_E_UNSUPPORTED
    refused(-7, params=params_with([4, 4, 1], cap_height=0))
    # a challenger whose input buffer is full can not have come from a plonky2 Challenger: SIPP_E_BADARG
    refused(-1, n_in=8)
    prove_and_compare(ctx, inst, devs, fc.challenger(case))                 # the ctx still proves
