"""sipp_prove_native_ex, sipp_flow_prove and sipp_flows_prove (sipp_amd/csrc/native.hip, flow.hip) on the GPU: the one-pass native chain
against the two calls it replaces (word for word), against the committed fixtures and against the Python verifier; every NULL
combination; refusals after which the same ctx works as before; the flow from points to the three STARK proofs against the stage-by-stage
proofs, alone and queued behind the producer thread; the C++ layer through tests/host/test_native_ex.cpp.

Sizes: n = 1 (no round), 2 (one round: the first-round shortcut only), 4 and 8 (the shortcut plus later cross_products rounds) and the
n = 128 fixture (the workload's size)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _pairing_cases as PC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, NOMEM, WITNESS = -1, -3, -8
SENTINEL = 0xA5A5A5A5
KEYS = ("g1", "g2", "fq12")


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=max(1 << 30, sipp_amd.lib().sipp_workspace_bytes(1, 64)))
    yield c
    c.close()


def fixture_points(n):
    A, B, _ = PC.fixture(n)
    return np.ascontiguousarray(A, dtype=np.uint32), np.ascontiguousarray(B, dtype=np.uint32)


_two_calls = {}


def two_calls(ctx, A, B):
    """(proof, accepted, statement, lists) of sipp_prove_native followed by sipp_verify_native: computed once per instance, never changed"""
    key = (A.tobytes(), B.tobytes())
    if key not in _two_calls:
        proof = ctx.prove_native(A, B)
        ok, st, ios = ctx.verify_native(A, B, proof)
        for a in [proof, st] + ios:
            a.setflags(write=False)
        _two_calls[key] = (proof, ok, st, ios)
    return _two_calls[key]


def assert_same(got, want, what):
    proof, ok, st, ios = got
    proof2, ok2, st2, ios2 = want
    assert proof.shape == proof2.shape and (proof == proof2).all(), (what, "proof")
    assert ok is ok2, (what, "accepted")
    assert st.shape == st2.shape and (st == st2).all(), (what, "statement")
    for g, w, key in zip(ios, ios2, KEYS):
        assert g.shape == w.shape and (g == w).all(), (what, key)


def assert_is_the_fixture(got, n):
    _, _, honest = PC.fixture(n)
    d = np.load(os.path.join(PC.GOLDEN, "sipp_n%d_ios.npz" % n))
    proof, ok, st, ios = got
    assert ok is True
    assert proof.shape == honest.shape and (proof == honest).all()
    assert st.shape == d["statement"].shape and (st == d["statement"]).all()
    for g, key in zip(ios, KEYS):
        assert g.shape == d[key].shape and (g == d[key]).all(), key


# ---------------- the one-pass chain ----------------
@pytest.mark.parametrize("n", [4, 8, 128])
def test_fixtures_and_the_two_calls(ctx, n):
    A, B, _ = PC.fixture(n)
    got = ctx.prove_native_ex(A, B)
    assert_is_the_fixture(got, n)
    assert_same(got, two_calls(ctx, A, B), "n = %d" % n)


@pytest.mark.parametrize("n", [1, 2])
def test_small_instances_and_the_python_verifier(ctx, n):
    A, B = PC.crafted_points(n)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    got = ctx.prove_native_ex(A, B)
    assert_same(got, two_calls(ctx, A, B), "n = %d" % n)
    proof, ok, st, ios = got
    ok2, st2, ios2 = PC.python_reading(A, B, proof)
    assert ok is True and ok2 is True
    assert (st == st2).all()
    for g, w, key in zip(ios, ios2, KEYS):
        assert g.shape == np.asarray(w).reshape(-1, g.shape[1]).shape and (g == np.asarray(w).reshape(-1, g.shape[1])).all(), key
    if n == 1:
        assert [a.shape for a in ios] == [(0, 56), (0, 104), (0, 296)]
        assert (st[:16] == st[48 + 96: 48 + 96 + 16]).all() and (st[16:48] == st[48 + 112: 48 + 144]).all()      # final = input
        assert (st[48: 48 + 96] == st[48 + 144:]).all() and (proof[0] == st[48: 48 + 96]).all()                  # final_Z = Z


def sentinel_buffers(n):
    import sipp_amd
    return {k: np.full(s, SENTINEL, dtype=np.uint32) for k, s in sipp_amd._lib.native_output_shapes(n).items()}


@pytest.mark.parametrize("lists,statement,check", [(False, False, False), (True, False, True), (True, True, False), (False, True, True)],
                         ids=["proof_only", "lists_without_statement", "all_but_accepted", "statement_without_lists"])
def test_null_combinations(ctx, lists, statement, check):
    """each output that is written equals the full call's; buffers of outputs that were not asked for keep their sentinel words"""
    A, B, _ = PC.fixture(4)
    full = ctx.prove_native_ex(A, B)
    out = sentinel_buffers(4)
    proof, ok, st, ios = ctx.prove_native_ex(A, B, lists=lists, check=check, statement=statement, out=out)
    assert proof is out["proof"] and (proof == full[0]).all()
    assert (ok is full[1]) if check else ok is None
    if statement:
        assert st is out["statement"] and (st == full[2]).all()
    else:
        assert st is None and (out["statement"] == SENTINEL).all()
    for i, key in enumerate(KEYS):
        if lists:
            assert ios[i] is out[key] and (ios[i] == full[3][i]).all(), key
        else:
            assert ios is None and (out[key] == SENTINEL).all(), key


def test_null_proof_and_single_lists_through_the_c_call(ctx):
    """the C entry with proof = NULL and one list at a time: the list asked for is the full call's, nothing else is written"""
    A, B = fixture_points(4)
    full = ctx.prove_native_ex(A, B)
    for i, key in enumerate(KEYS):
        out = sentinel_buffers(4)
        ptrs = [out[k].ctypes.data if k == key else None for k in KEYS]
        rc = ctx.L.sipp_prove_native_ex(ctx.h, A.ctypes.data, B.ctypes.data, 4, None, None, ptrs[0], ptrs[1], ptrs[2], None)
        assert rc == 0
        assert (out[key] == full[3][i]).all(), key


def test_the_lists_feed_the_provers(ctx):
    """Instance.prove on the lists of the one-pass chain: the oracle's proofs of the n = 4 fixture, by digest"""
    import sipp_amd
    A, B, _ = PC.fixture(4)
    ios = ctx.prove_native_ex(A, B)[3]
    gold = json.load(open(os.path.join(PC.GOLDEN, "proof_digests_n4.json")))
    inst = sipp_amd.Instance([a.shape[0] for a in ios])
    try:
        proofs = inst.prove(ios)
        for pf, key in zip(proofs, KEYS):
            if key in gold:
                assert len(pf) == gold[key]["words"] and hashlib.sha256(pf.tobytes()).hexdigest() == gold[key]["sha256"], key
    finally:
        inst.close()


# ---------------- refusals (host refusals and device error flags: no fault) ----------------
def refused_points():
    """[(name, A)]: the n = 4 fixture's A with infinity as a fold's offset (A1) and as its base (A2), and with a point off its curve"""
    A, _, _ = PC.fixture(4)
    out = []
    for name, row in (("infinity_in_A1", 1), ("infinity_in_A2", 3)):
        bad = A.copy()
        bad[row] = 0
        out.append((name, bad))
    bad = A.copy()
    bad[2, 8] ^= 1
    out.append(("off_curve_in_A2", bad))
    return out


def test_refused_witnesses_leave_the_ctx_usable(ctx):
    import sipp_amd
    A, B, _ = PC.fixture(4)
    for name, bad in refused_points():
        for kw in ({}, {"lists": False, "statement": False, "check": False}):
            with pytest.raises(sipp_amd.SippError) as e:
                ctx.prove_native_ex(bad, B, **kw)
            assert e.value.code == WITNESS, name
            assert_is_the_fixture(ctx.prove_native_ex(A, B), 4)


@pytest.mark.parametrize("n", [3, 6])
def test_sizes_that_are_no_power_of_two(ctx, n):
    import sipp_amd
    A8, B8 = fixture_points(8)
    A, B = np.ascontiguousarray(A8[:n]), np.ascontiguousarray(B8[:n])
    out = sentinel_buffers(8)
    rc = ctx.L.sipp_prove_native_ex(ctx.h, A.ctypes.data, B.ctypes.data, n, out["proof"].ctypes.data, out["statement"].ctypes.data,
                                    out["g1"].ctypes.data, out["g2"].ctypes.data, out["fq12"].ctypes.data, None)
    assert rc == BADARG and all((a == SENTINEL).all() for a in out.values())
    with pytest.raises(sipp_amd.SippError) as e:
        ctx.prove_native_ex(A, B)
    assert e.value.code == BADARG
    assert_is_the_fixture(ctx.prove_native_ex(*PC.fixture(4)[:2]), 4)


def test_a_workspace_for_the_fold_but_not_for_the_fq12_powers():
    """1 MiB at n = 4 holds the fold (2 records: 2 x 512 rows of 192 + 384 bytes, and the records) but not the Fq12 trace of the 4 powers:
    SIPP_E_NOMEM whenever final_Z is needed (lists, statement or accepted), success when only the proof (or the G1 / G2 lists, which
    the fold leaves behind) is asked for; the ctx is usable after each"""
    import sipp_amd
    (A, B), honest = fixture_points(4), PC.fixture(4)[2]
    d = np.load(os.path.join(PC.GOLDEN, "sipp_n4_ios.npz"))
    workspace = 1 << 20
    small = sipp_amd.Ctx(workspace_bytes=workspace)
    try:
        log_n, width = small.shape(2, 4)[:2]
        assert (width * 8) << log_n > workspace > 2 * 512 * (192 + 384) + 2 * 4 * (56 + 104) + 1024
        for kw in ({}, {"lists": False, "statement": False}, {"lists": False, "check": False}):
            with pytest.raises(sipp_amd.SippError) as e:
                small.prove_native_ex(A, B, **kw)
            assert e.value.code == NOMEM, kw
            proof, ok, st, ios = small.prove_native_ex(A, B, lists=False, statement=False, check=False)
            assert (proof == honest).all() and ok is None and st is None and ios is None
        g1, g2 = np.zeros_like(d["g1"]), np.zeros_like(d["g2"])
        assert small.L.sipp_prove_native_ex(small.h, A.ctypes.data, B.ctypes.data, 4, None, None, g1.ctypes.data, g2.ctypes.data, None, None) == 0
        assert (g1 == d["g1"]).all() and (g2 == d["g2"]).all()
        assert (small.prove_native(A, B) == honest).all()
    finally:
        small.close()


# ---------------- from the points to the three proofs ----------------
def rolled(n, k):
    A, B = fixture_points(n)
    return np.ascontiguousarray(np.roll(A, k, axis=0)), np.ascontiguousarray(np.roll(B, k, axis=0))


@pytest.fixture(scope="module")
def stage_by_stage(ctx):
    """instance -> (three proofs, native proof, statement) through prove_native, verify_native and Instance.prove on ctxs of their own;
    computed once per instance"""
    import sipp_amd
    insts, cache = {}, {}

    def get(A, B):
        key = (A.tobytes(), B.tobytes())
        if key not in cache:
            proof, ok, st, ios = two_calls(ctx, A, B)
            assert ok
            num_io = tuple(a.shape[0] for a in ios)
            if num_io not in insts:
                insts[num_io] = sipp_amd.Instance(num_io)
            proofs = [p.copy() for p in insts[num_io].prove(ios)]
            for p in proofs:
                p.setflags(write=False)
            cache[key] = (proofs, proof, st)
        return cache[key]

    yield get
    for i in insts.values():
        i.close()


def assert_same_flow(got, want, what):
    proofs, nproof, st, ok = got
    assert ok is True, what
    assert (nproof == want[1]).all() and (st == want[2]).all(), what
    for k in range(3):
        assert len(proofs[k]) == len(want[0][k]) and (proofs[k] == want[0][k]).all(), (what, k)


@pytest.mark.parametrize("n", [4, 8])
def test_flow_gives_the_stage_by_stage_proofs(stage_by_stage, n):
    import sipp_amd
    from tests import _verify
    A, B, honest = PC.fixture(n)
    d = np.load(os.path.join(PC.GOLDEN, "sipp_n%d_ios.npz" % n))
    inst = sipp_amd.Instance([n - 1, n - 1, 2 * (n.bit_length() - 1)])
    try:
        got = inst.flow(inst.ctxs[1], A, B)            # the native chain on the G2 ctx: one of the three
        assert_same_flow(got, stage_by_stage(A, B), "n = %d" % n)
        assert (got[1] == honest).all() and (got[2] == d["statement"]).all()
        for pf in got[0]:
            assert _verify.both_accept(pf)
    finally:
        inst.close()


def test_queued_flows(ctx, stage_by_stage):
    """five instances through two slots behind the producer: the four rolled copies of the n = 4 fixture are word for word their
    stage-by-stage proofs; the one with infinity among its points is refused with SIPP_E_WITNESS, alone"""
    import sipp_amd
    good = [rolled(4, k) for k in range(4)]
    badA = good[0][0].copy()
    badA[2] = 0
    instances = [good[0], good[1], (badA, good[0][1]), good[2], good[3]]
    q = sipp_amd.InstanceQueue([3, 3, 4], in_flight=2)
    try:
        rc, status, res = q.flows(ctx, instances, raise_on_error=False)
        assert rc == WITNESS and status == [0, 0, WITNESS, 0, 0]
        assert [len(p) for p in res[2][0]] == [0, 0, 0]
        for i in (0, 1, 3, 4):
            assert_same_flow(res[i], stage_by_stage(*instances[i]), "instance %d" % i)
        with pytest.raises(sipp_amd.SippError) as e:
            q.flows(ctx, instances)
        assert e.value.code == WITNESS
        five = good + [good[0]]
        for i, r in enumerate(q.flows(ctx, five)):      # the same objects, SIPP_OK
            assert_same_flow(r, stage_by_stage(*five[i]), "second call, instance %d" % i)
        assert q.flows(ctx, []) == []
        with pytest.raises(sipp_amd.SippError) as e:
            q.flows(q.slots[1].ctxs[2], [good[0]])
        assert e.value.code == BADARG
    finally:
        q.close()


def test_a_queue_of_one_is_the_flow(ctx, stage_by_stage):
    import sipp_amd
    A, B = rolled(4, 1)
    q = sipp_amd.InstanceQueue([3, 3, 4], in_flight=1)
    try:
        res = q.flows(ctx, [(A, B)])
        assert len(res) == 1
        lone = q.slots[0].flow(ctx, A, B)
        assert_same_flow(res[0], ([p.copy() for p in lone[0]], lone[1], lone[2]), "queue of one")
        assert_same_flow(res[0], stage_by_stage(A, B), "queue of one, stage by stage")
    finally:
        q.close()


# ---------------- the C++ layer ----------------
def test_cpp_layer(tmp_path):
    """sipp::Prover::sipp_prove_native_ex at n = 4 equals sipp_prove_native + sipp_verify_native (tests/host/test_native_ex.cpp)"""
    import sipp_amd
    sipp_amd.lib()
    exe = str(tmp_path / "test_native_ex")
    lib = os.path.join(ROOT, "sipp_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_native_ex.cpp"), "-L" + lib, "-lsipp_hip", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib"])
    A, B, _ = PC.fixture(4)
    with open(tmp_path / "points.bin", "wb") as f:
        f.write(np.array([4], dtype=np.uint32).tobytes() + np.ascontiguousarray(A).tobytes() + np.ascontiguousarray(B).tobytes())
    out = subprocess.run([exe, str(tmp_path / "points.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "native_ex ok: 4 pairs" in out.stdout, out.stdout + out.stderr
