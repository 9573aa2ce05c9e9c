"""sipp_prove_native_ex, sipp_flow_prove and sipp_flows_prove without a GPU: the argument refusals that return before a ctx is touched
(SIPP_E_BADARG; the handles below are never dereferenced on these paths) and the shape checks of the Python wrappers, which raise before
any call into the library."""
import ctypes as C

import numpy as np
import pytest

import sipp_amd
from sipp_amd import _lib

BADARG = -1
vp = C.c_void_p


def handles(*values):
    return (vp * len(values))(*values)


@pytest.fixture(scope="module")
def L():
    return sipp_amd.lib()


@pytest.fixture(scope="module")
def points():
    A, B = np.zeros((4, 16), dtype=np.uint32), np.zeros((4, 32), dtype=np.uint32)
    return A, B


def test_prove_native_ex_refuses_null_arguments(L, points):
    A, B = points
    proof = np.full((5, 96), 7, dtype=np.uint32)
    assert L.sipp_prove_native_ex(None, A.ctypes.data, B.ctypes.data, 4, proof.ctypes.data, None, None, None, None, None) == BADARG
    assert L.sipp_prove_native_ex(vp(1), None, B.ctypes.data, 4, proof.ctypes.data, None, None, None, None, None) == BADARG
    assert L.sipp_prove_native_ex(vp(1), A.ctypes.data, None, 4, proof.ctypes.data, None, None, None, None, None) == BADARG
    assert (proof == 7).all()


def test_flow_prove_refuses_null_arguments(L, points):
    A, B = points
    ctxs = handles(1, 2, 3)
    out = [np.zeros(8, dtype=np.uint64) for _ in range(3)]
    po = handles(*[o.ctypes.data for o in out])
    pc = (C.c_size_t * 3)(8, 8, 8)
    pl = (C.c_size_t * 3)(5, 5, 5)
    good = [vp(4), ctxs, A.ctypes.data, B.ctypes.data, 4, None, None, po, pc, pl, None]
    for i in (0, 1, 2, 3, 7, 8, 9):
        args = list(good)
        args[i] = None
        assert L.sipp_flow_prove(*args) == BADARG, i
    args = list(good)
    args[1] = handles(1, None, 3)
    assert L.sipp_flow_prove(*args) == BADARG
    assert list(pl) == [5, 5, 5]


def flows_args(points, count=1, in_flight=1, native=9, slots=(1, 2, 3)):
    A, B = points
    out = [np.zeros(8, dtype=np.uint64) for _ in range(3 * max(count, 1))]
    keep = (out,)
    return [vp(native), handles(*slots), in_flight, count, 4, handles(*[A.ctypes.data] * max(count, 1)), handles(*[B.ctypes.data] * max(count, 1)),
            None, None, handles(*[o.ctypes.data for o in out]), (C.c_size_t * len(out))(*[8] * len(out)), (C.c_size_t * len(out))(), None,
            None], keep


def test_flows_prove_refuses_bad_arguments_before_anything_starts(L, points):
    good, keep = flows_args(points)
    for i in (0, 1, 5, 6, 9, 10, 11):                      # native_ctx, ctxs, A, B, proof_out, proof_cap, proof_len
        args = list(good)
        args[i] = None
        assert L.sipp_flows_prove(*args) == BADARG, i
    args = list(good)
    args[2] = 0                                            # no slot
    assert L.sipp_flows_prove(*args) == BADARG
    for slots in ((1, None, 3), (1, 2, 1), (1, 9, 3)):     # a NULL slot ctx, a duplicate, the native ctx among the slots
        args, keep2 = flows_args(points, slots=slots)
        assert L.sipp_flows_prove(*args) == BADARG, slots
    args, keep2 = flows_args(points, in_flight=2, slots=(1, 2, 3, 4, 5, 9))
    assert L.sipp_flows_prove(*args) == BADARG
    for i in (5, 6, 9):                                    # a NULL A[0] / B[0] / proof_out[0]
        args = list(good)
        args[i] = handles(None) if i != 9 else handles(None, None, None)
        assert L.sipp_flows_prove(*args) == BADARG, i
    del keep, keep2


def test_flows_prove_takes_an_empty_queue(L, points):
    args, keep = flows_args(points, count=0)
    assert L.sipp_flows_prove(*args) == 0
    args[5] = args[6] = args[9] = args[10] = args[11] = None          # with count = 0 the instance arrays are not read
    assert L.sipp_flows_prove(*args) == 0
    args[1] = handles(1, 2, 9)                                        # ... but the slots are still checked
    assert L.sipp_flows_prove(*args) == BADARG
    del keep


# ---------------- the Python wrappers' shape checks ----------------
def test_native_points_shapes():
    A, B = np.zeros((8, 16), dtype=np.uint32), np.zeros((8, 32), dtype=np.uint32)
    a, b, n, lg = _lib.native_points(A, B)
    assert (n, lg) == (8, 3) and a.shape == (8, 16) and b.shape == (8, 32)
    a, b, n, lg = _lib.native_points(A.reshape(-1), B.reshape(-1).tolist())
    assert (n, lg) == (8, 3) and b.dtype == np.uint32
    assert _lib.native_points(A[:1], B[:1])[2:] == (1, 0)
    for bad_a, bad_b in ((A[:3], B[:3]), (A[:6], B[:6]), (A, B[:4]), (A[:0], B[:0]), (np.zeros(17, dtype=np.uint32), B[:1]),
                         (A[:2], np.zeros(33, dtype=np.uint32))):
        with pytest.raises(sipp_amd.SippError) as e:
            _lib.native_points(bad_a, bad_b)
        assert e.value.code == BADARG


def test_native_output_shapes_are_the_headers():
    assert _lib.native_output_shapes(1) == {"proof": (1, 96), "statement": (288,), "g1": (0, 56), "g2": (0, 104), "fq12": (0, 296)}
    assert _lib.native_output_shapes(128) == {"proof": (15, 96), "statement": (48 * 128 + 240,), "g1": (127, 56), "g2": (127, 104), "fq12": (14, 296)}
    L = sipp_amd.lib()
    for n in (1, 2, 4, 128, 4096):
        shp = _lib.native_output_shapes(n)
        assert shp["proof"][0] * 96 == L.sipp_native_proof_words(n)


def test_caller_buffers_are_checked():
    ok = np.zeros((3, 56), dtype=np.uint32)
    assert _lib._native_out({"g1": ok}, "g1", (3, 56), "t") is ok
    fresh = _lib._native_out({"g2": ok}, "g1", (3, 56), "t")
    assert fresh is not ok and fresh.shape == (3, 56) and fresh.dtype == np.uint32 and not fresh.any()
    assert _lib._native_out(None, "g1", (0, 56), "t").shape == (0, 56)
    ro = np.zeros((3, 56), dtype=np.uint32)
    ro.setflags(write=False)
    for bad in (np.zeros((3, 56), dtype=np.uint64), np.zeros((4, 56), dtype=np.uint32), np.zeros((56, 3), dtype=np.uint32).T, ro, [[0] * 56] * 3):
        with pytest.raises(sipp_amd.SippError) as e:
            _lib._native_out({"g1": bad}, "g1", (3, 56), "t")
        assert e.value.code == BADARG


def test_wrappers_exist_where_the_issue_puts_them():
    assert callable(sipp_amd.Ctx.prove_native_ex) and callable(sipp_amd.Instance.flow) and callable(sipp_amd.InstanceQueue.flows)
