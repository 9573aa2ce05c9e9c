"""The pairing products (sipp_inner_product(s): miller_kernel, product_kernel, final_exp_kernel of sipp_amd/csrc/pairing.hip) and the native
chain's host side (sipp_amd/csrc/native.hip) on the GPU against the catalogue tests/_pairing_cases.py, which tests/test_oracle_pairing_cases.py
pins on the CPU: every group word for word (edge coordinates, the three infinity shapes, products that are exactly ONE, 255 .. 513 pairs
and group offsets 257 k against a closed form the device has no part in), crafted and tampered proofs against the Python reading of the
verifier, refusals after which the same ctx must work as before, and the argument errors of the products (host refusals: none of them
launches a kernel)."""
import ctypes as C

import numpy as np
import pytest

from tests import _pairing_cases as PC

pytestmark = pytest.mark.gpu
BADARG, NOMEM, WITNESS = -1, -3, -8


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def run(ctx, case):
    g1, g2, count, want = PC.case_words(case)
    return ctx.inner_products(g1, g2, count=count), want


def differing(cases, results):
    return ["%s[group %d]" % (c.name, k) for c, (got, want) in zip(cases, results) for k in np.flatnonzero((got != want).any(axis=1))]


def assert_reproduces_the_fixture(ctx, n=4):
    A, B, honest = PC.fixture(n)
    d = np.load("tests/golden/sipp_n%d_ios.npz" % n)
    proof = ctx.prove_native(A, B)
    assert (proof == honest).all()
    ok, st, ios = ctx.verify_native(A, B, proof)
    assert ok and (st == d["statement"]).all()
    for got, key in zip(ios, ("g1", "g2", "fq12")):
        assert got.shape == d[key].shape and (got == d[key]).all(), key


def assert_same_reading(got, want, what):
    ok, st, ios = got
    ok2, st2, ios2 = want
    assert ok == ok2, what
    assert (st == st2).all(), "%s: statement words %s differ" % (what, np.flatnonzero(st != st2)[:8].tolist())
    for g, w, key in zip(ios, ios2, ("g1", "g2", "fq12")):
        assert g.shape == w.shape and (g == w).all(), (what, key)


# ---------------- the products ----------------
def test_small_groups_match_the_catalogue(ctx):
    cases = PC.small_cases_recorded()
    bad = differing(cases, [run(ctx, c) for c in cases])
    assert not bad, bad


def test_size_cases_match_the_closed_form_twice(ctx):
    """255 .. 513 pairs, with infinity pairs at 0 / 255 / 256 / n - 1, a single finite pair at the last index, and 3 / 5 groups of 257
    (offsets 257 k); every call is made twice: the same words both times"""
    cases = PC.size_cases()
    first = [run(ctx, c) for c in cases]
    bad = differing(cases, first)
    assert not bad, bad
    again = [run(ctx, c) for c in cases]
    assert all((a[0] == b[0]).all() for a, b in zip(first, again))


def test_product_does_not_depend_on_the_order_of_the_pairs(ctx):
    case = next(c for c in PC.size_cases() if c.name == "size_513")
    g1, g2, _, want = PC.case_words(case)
    assert (ctx.inner_products(g1[::-1], g2[::-1]) == want).all()
    case = next(c for c in PC.size_cases() if c.name == "lone_pair_of_257")                 # the finite pair first instead of last
    g1, g2, _, want = PC.case_words(case)
    assert (ctx.inner_products(g1[::-1], g2[::-1]) == want).all()


# ---------------- the verifier's host arithmetic on crafted messages ----------------
def test_crafted_proofs_match_the_python_reading(ctx):
    for name, n, proof in PC.crafted_proofs():
        A, B = PC.crafted_points(n)
        want = PC.python_reading(A, B, proof)
        assert want[0] is False
        assert_same_reading(ctx.verify_native(A, B, PC.proof_words(proof)), want, name)


def test_tamper_table_is_rejected(ctx):
    A, B, honest = PC.fixture(8)
    assert (ctx.prove_native(A, B) == honest).all()
    accepted = []
    for name, _, pf in PC.tampered_proofs():
        got = ctx.verify_native(A, B, pf)
        if got[0]:
            accepted.append(name)
        if name in PC.READ_TAMPERED:
            assert_same_reading(got, PC.python_reading(A, B, pf), name)
    assert not accepted, accepted
    assert ctx.verify_native(A, B, honest)[0]


# ---------------- refusals and what they leave behind ----------------
def bad_inputs():
    """[(name, A)]: the n = 4 fixture's A with infinity as a fold's offset (A1) and as its base (A2), and with a point off the curve"""
    A, _, _ = PC.fixture(4)
    out = []
    for name, i in (("infinity_in_A1", 1), ("infinity_in_A2", 3)):
        bad = A.copy()
        bad[i] = 0
        out.append((name, bad))
    bad = A.copy()
    bad[2, 8] ^= 1                                                   # y +- 1
    out.append(("off_curve_in_A2", bad))
    return out


def test_refused_inputs_and_the_ctx_afterwards(ctx):
    """the refused fold after sipp_fold_begin (prove: after the products; verify: after the Fq12 powers): SIPP_E_WITNESS, and the SAME ctx
    then reproduces the n = 4 fixture -- no fold left in flight, the arena handed back"""
    import sipp_amd
    _, B, honest = PC.fixture(4)
    assert_reproduces_the_fixture(ctx)
    for name, bad in bad_inputs():
        for call in (lambda: ctx.prove_native(bad, B), lambda: ctx.verify_native(bad, B, honest)):
            with pytest.raises(sipp_amd.SippError) as e:
                call()
            assert e.value.code == WITNESS, name
            assert_reproduces_the_fixture(ctx)


def test_zero_message_is_taken_and_read_as_python_reads_it(ctx):
    """Z_L = 0 is NOT refused: the Fq12 AIR proves records with the base 0 (tests/_exp_edges.py has them: zero__one__e0, zero_zero_0), so
    sipp_exp_outputs takes (x = 0, offset = 1, exp_val = the round's challenge) and returns 0, and sipp_verify_native reads the proof as
    the Python verifier does: Z Z_L^x = 0 from there on, not accepted"""
    n, proof = PC.zero_message_proof()
    A, B = PC.crafted_points(n)
    want = PC.python_reading(A, B, proof)
    assert want[0] is False and not want[1][-96:].any()
    rec = np.zeros((1, 296), dtype=np.uint32)
    rec[0, 96] = 1
    rec[0, 192:200] = want[2][2][0, 192:200]
    assert not ctx.exp_outputs(2, rec)[0, 200:].any()
    assert_same_reading(ctx.verify_native(A, B, PC.proof_words(proof)), want, "zero message")
    assert_reproduces_the_fixture(ctx)


def test_failing_fq12_powers_drain_the_fold_begun_before_them():
    """sipp_verify_native begins the first round's fold (side streams, arena blocks held) BEFORE the Fq12 powers; when those fail it has to
    drain the fold and hand the arena back.  No record of the catalogue makes sipp_exp_outputs(SIPP_FQ12_EXP) refuse (zero is proved, see
    above), so the failure here is a host refusal: a workspace of 1 MiB holds the n = 4 fold (2 records: 2 x 512 rows of 192 + 384 bytes
    = 576 KiB, and the records) but not the Fq12 trace of the 4 powers -> SIPP_E_NOMEM after sipp_fold_begin.  The same ctx then
    proves the n = 4 fixture again, which begins a fold of the same size: it would be refused (a fold in flight) or find the arena
    short if the drain had not happened"""
    import sipp_amd
    A, B, honest = PC.fixture(4)
    workspace = 1 << 20
    small = sipp_amd.Ctx(workspace_bytes=workspace)
    try:
        log_n, width = small.shape(2, 4)[:2]
        assert (width * 8) << log_n > workspace > 2 * 512 * (192 + 384) + 2 * 4 * (56 + 104) + 1024
        assert (small.prove_native(A, B) == honest).all()                    # the fold fits
        for _ in range(2):
            with pytest.raises(sipp_amd.SippError) as e:
                small.verify_native(A, B, honest)
            assert e.value.code == NOMEM
            assert (small.prove_native(A, B) == honest).all()
    finally:
        small.close()


# ---------------- argument errors of the products: host refusals ----------------
def raw_products(ctx, n, count, pairs=1):
    case = PC.small_cases_recorded()[0]
    g1, g2, _, _ = PC.case_words(case)
    g1, g2 = np.ascontiguousarray(np.repeat(g1, pairs, axis=0)), np.ascontiguousarray(np.repeat(g2, pairs, axis=0))
    out = np.zeros((1, 96), dtype=np.uint32)
    return ctx.L.sipp_inner_products(ctx.h, g1.ctypes.data, g2.ctypes.data, C.c_size_t(n), C.c_size_t(count), out.ctypes.data), out


@pytest.mark.parametrize("n,count", [(0, 1), (1, 0), ((1 << 12) + 1, 1 << 12), ((1 << 24) + 1, 1), (1, (1 << 24) + 1), (1 << 40, 1 << 24), (1 << 63, 2)],
                         ids=["n0", "count0", "above_2p24", "n_above_2p24", "count_above_2p24", "wraps_to_0", "wraps_to_0_top_bit"])
def test_products_refuse_bad_sizes_before_reading_anything(ctx, n, count):
    """one valid pair is all the buffers hold: the call must return before it sizes anything by n or count (n count wraps to 0 for
    2^40 x 2^24)"""
    rc, out = raw_products(ctx, n, count)
    assert rc == BADARG and not out.any()
    got, want = run(ctx, PC.small_cases_recorded()[0])
    assert (got == want).all()


def test_products_beyond_the_workspace_are_refused_and_the_ctx_survives():
    """any non-zero workspace is accepted; 4096 bytes hold the one-pair product (five blocks at multiples of 256: 1544 bytes) but not 8
    pairs (64 + 128 + 384 = 576 bytes each, 4608 in all)"""
    import sipp_amd
    small = sipp_amd.Ctx(workspace_bytes=4096)
    try:
        pairs = 4096 // 576 + 1
        rc, out = raw_products(small, pairs, 1, pairs=pairs)
        assert rc == NOMEM and not out.any()
        got, want = run(small, PC.small_cases_recorded()[0])
        assert (got == want).all()
    finally:
        small.close()
