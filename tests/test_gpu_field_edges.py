"""The device arithmetic itself at its carry and bound edges: the product's own headers (gl.hpp, gl_lazy.hpp and its generated
interleaved block, fq.hpp, poseidon.hpp, poseidon_pair.hpp) instantiated in the elementwise kernels of tests/probe/field_probe.hip and
compared, element by element, with exact Python integers.

Random field elements reach the rare paths of these functions -- a carry out of the top word, a borrow in the hand-scheduled product,
an accumulator filled to its limit, an all-0x00 or all-0xFF byte plane in the matrix-pipe layers -- with probability near 2^-32 per
operation, so the whole-proof parity tests cannot see them.  Here every function is fed the lattice of word values where carries and
borrows flip, inside the domain its comment documents: a `_nc` result must be congruent to the exact value, a canonical one equal to it.
Element counts are not multiples of 64, so partial waves run too (the matrix-pipe probes run whole waves, as the product's kernels do:
MFMA ignores EXEC)."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tests", "probe")
P = 2**64 - 2**32 + 1
M64 = 2**64 - 1
N_RANDOM = (1 << 20) + 13            # random cases per cheap op: not a multiple of 64


# ---------------------------------------------------------------------------------------------------------------------------------
# the probe library

class Probe:
    """tests/probe/libfield_probe.so through ctypes; numpy uint64 arrays in and out (the device buffers are torch tensors)"""

    def __init__(self):
        import torch  # noqa: F401  (first: the probe binds to torch's HIP runtime, as sipp_amd._lib does)
        subprocess.check_call(["make", "-C", PROBE_DIR, "-s"])
        L = C.CDLL(os.path.join(PROBE_DIR, "libfield_probe.so"))
        u64, vp = C.c_uint64, C.c_void_p
        sig = {
            "probe_init": [],
            "probe_dense_mats": [],
            "probe_gl": [C.c_int, vp, vp, vp, vp, u64],
            "probe_gll": [C.c_int, vp, vp, vp, u64],
            "probe_acc": [C.c_int, vp, vp, vp, C.c_uint32, vp, u64],
            "probe_fq": [C.c_int, vp, vp, vp, u64],
            "probe_poseidon": [C.c_int, C.c_uint32, vp, vp, vp, u64],
        }
        for name, args in sig.items():
            getattr(L, name).restype = C.c_int
            getattr(L, name).argtypes = args
        assert L.probe_init() == 0, "probe_init: uploading the Poseidon tables failed"
        self.L = L
        self.dense_mats = L.probe_dense_mats()

    @staticmethod
    def _dev(a):
        from sipp_amd._lib import to_device
        return to_device(np.ascontiguousarray(a, dtype=np.uint64).ravel())

    def _run(self, fn, head, arrays, out_words, n):
        import torch
        from sipp_amd._lib import to_host
        devs = [self._dev(a) for a in arrays]
        out = torch.zeros(max(out_words, 1), dtype=torch.int64, device="cuda")
        rc = fn(*head, *[d.data_ptr() for d in devs], out.data_ptr(), n)
        assert rc == 0, "%s returned hipError %d" % (fn.__name__, rc)
        return to_host(out)[:out_words]

    def gl(self, op, a, b=None, c=None, width=1):
        n = len(a) // width
        b = a if b is None else b
        c = a[:n] if c is None else c
        assert len(b) == len(a) and len(c) == n
        return self._run(self.L.probe_gl, (op,), [a, b, c], len(a), n)

    def gll(self, op, a, b=None, width=1):
        n = len(a) // width
        b = a if b is None else b
        assert len(b) == len(a)
        return self._run(self.L.probe_gll, (op,), [a, b], len(a), n)

    def acc(self, op, start, x, y, terms):
        n = len(start) // 2
        assert x.shape == (terms, n) and y.shape == (terms, n)
        devs = [self._dev(v) for v in (start, x, y)]
        import torch
        from sipp_amd._lib import to_host
        out = torch.zeros(n, dtype=torch.int64, device="cuda")
        rc = self.L.probe_acc(op, devs[0].data_ptr(), devs[1].data_ptr(), devs[2].data_ptr(), terms, out.data_ptr(), n)
        assert rc == 0, "probe_acc returned hipError %d" % rc
        return to_host(out)

    def fq(self, op, a, b=None, width=4):
        n = len(a) // width
        b = a if b is None else b
        assert len(b) == len(a)
        return self._run(self.L.probe_fq, (op,), [a, b], len(a), n)

    def poseidon(self, op, states, arg=0, addend=None):
        states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 12)
        n = states.shape[0]
        addend = states[:, :11] if addend is None else np.asarray(addend, dtype=np.uint64).reshape(n, 11)
        return self._run(self.L.probe_poseidon, (op, arg), [states, addend], 12 * n, n).reshape(n, 12)


@pytest.fixture(scope="module")
def probe():
    return Probe()


# op codes (tests/probe/field_probe.hip)
GL = dict(add=0, sub=1, neg=2, dbl=3, mul=4, mul_nc=5, mad_nc=6, add_nc=7, reduce128_nc=8, reduce96_nc=9, inv=10, pow=11, root=12,
          canon=13, reduce128=14, reduce96=15, sqr=16, mad=17, e2_mul=32, e2_sqr=33, e2_inv=34, e2_pow=35)
GLL = dict(canon=0, add_nc=1, sub_nc=2, mul_nc=3, reduce96_nc=4, reduce128_nc=5, mul3_nc=6)
FQ = dict(add=0, sub=1, neg=2, dbl=3, mul=4, sqr=5, to_mont=6, from_mont=7, inv=8, inv_gcd=9, is_zero=10,
          fq2_add=16, fq2_sub=17, fq2_mul=18, fq2_sqr=19, fq2_inv=20, fq2_inv_gcd=21)
PSN = dict(mds=0, mds_add=1, mds_mfma=2, mds_mfma_add=3, dense=4, dense_addend=5, permute=6, permute_mfma=7)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact references and comparison

def obj(a):
    """uint64 array -> array of Python ints"""
    return np.asarray(a, dtype=np.uint64).astype(object)


def u64(vals):
    return np.array([int(v) for v in vals], dtype=np.uint64)


def _fmt(v):
    return hex(int(v)) if not isinstance(v, (tuple, list, np.ndarray)) else "(" + ", ".join(hex(int(x)) for x in np.ravel(v)) + ")"


def check(got, want, what, inputs=(), exact=True, mod=P):
    """got (uint64) against want (Python ints, canonical): equal (exact) or congruent mod `mod`; names the first failing inputs"""
    g = obj(got)
    bad = (g != want) if exact else (g % mod != want)
    idx = np.flatnonzero(np.asarray(bad, dtype=bool))
    if len(idx):
        i = idx[0]
        ins = ", ".join("%s" % _fmt(np.asarray(x)[i]) for x in inputs)
        raise AssertionError("%s: %d of %d wrong; first at %d: inputs %s -> got %s, want %s%s" % (
            what, len(idx), len(g), i, ins, _fmt(g[i]), "" if exact else "congruent to ", _fmt(want[i])))


# ---------------------------------------------------------------------------------------------------------------------------------
# the Goldilocks edge lattice

WORDS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
NAMED = [0, 1, 2**32 - 1, 2**32, 2**63, P - 2, P - 1, P, P + 1, 2**64 - 2, 2**64 - 1]
EDGE_ANY = sorted({(h << 32) | l for h in WORDS for l in WORDS} | {v + d for v in NAMED for d in range(-3, 4) if 0 <= v + d <= M64})
EDGE_CANON = [v for v in EDGE_ANY if v < P]


def rand_any(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)


def rand_canon(rng, n):
    return rng.integers(0, P, size=n, dtype=np.uint64, endpoint=False)


def cross(xs, ys):
    a, b = zip(*itertools.product(xs, ys))
    return u64(a), u64(b)


def binary_cases(seed, a_dom, b_dom, n_random=N_RANDOM):
    """the full edge cross product, then n_random random pairs from the two domains ('any' u64 or 'canon')"""
    ea, eb = cross(EDGE_ANY if a_dom == "any" else EDGE_CANON, EDGE_ANY if b_dom == "any" else EDGE_CANON)
    rng = np.random.default_rng(seed)
    ra = (rand_any if a_dom == "any" else rand_canon)(rng, n_random)
    rb = (rand_any if b_dom == "any" else rand_canon)(rng, n_random)
    return np.concatenate([ea, ra]), np.concatenate([eb, rb])


def unary_cases(seed, dom, n_random=N_RANDOM):
    rng = np.random.default_rng(seed)
    e = u64(EDGE_ANY if dom == "any" else EDGE_CANON)
    return np.concatenate([e, (rand_any if dom == "any" else rand_canon)(rng, n_random)])


def word_cases(k):
    """all 6^k combinations of the edge words, as (hi, lo) for k = 4 (128-bit) or (hi32, lo) for k = 3"""
    combos = list(itertools.product(WORDS, repeat=k))
    if k == 4:
        return u64([(w[0] << 32) | w[1] for w in combos]), u64([(w[2] << 32) | w[3] for w in combos])
    return u64([w[0] for w in combos]), u64([(w[1] << 32) | w[2] for w in combos])


# ---------------------------------------------------------------------------------------------------------------------------------
# gl:: (gl.hpp)

@pytest.mark.parametrize("op", ["add", "sub", "mul", "mul_nc", "add_nc", "mad", "mad_nc"])
def test_gl_binary_ops_on_the_edge_lattice(probe, op):
    """add / sub: canonical x canonical, exact.  mul / mul_nc: any u64 x any u64 (exact / congruent).  add_nc: any u64 + canonical.
    mad / mad_nc: any u64 x any u64 + any u64 (the addend runs over the lattice shifted against the factors)"""
    dom = {"add": ("canon", "canon"), "sub": ("canon", "canon"), "add_nc": ("any", "canon")}.get(op, ("any", "any"))
    a, b = binary_cases(10 + GL[op], *dom)
    A, B = obj(a), obj(b)
    c = None
    if op in ("mad", "mad_nc"):
        c = np.roll(np.concatenate([u64(EDGE_ANY)] * (len(a) // len(EDGE_ANY) + 1))[: len(a)], 7)
        c[-N_RANDOM:] = rand_any(np.random.default_rng(3), N_RANDOM)
        want = (A * B + obj(c)) % P
    else:
        want = {"add": (A + B) % P, "sub": (A - B) % P, "add_nc": (A + B) % P}.get(op, (A * B) % P)
    got = probe.gl(GL[op], a, b, c)
    check(got, want, "gl::" + op, (a, b) if c is None else (a, b, c), exact=not op.endswith("_nc"))


@pytest.mark.parametrize("op", ["neg", "dbl", "canon", "sqr"])
def test_gl_unary_ops_on_the_edge_lattice(probe, op):
    """neg / dbl: canonical in; canon / sqr: any u64 in; all exact"""
    a = unary_cases(30 + GL[op], "canon" if op in ("neg", "dbl") else "any")
    A = obj(a)
    want = {"neg": (-A) % P, "dbl": (2 * A) % P, "canon": A % P, "sqr": (A * A) % P}[op]
    check(probe.gl(GL[op], a), want, "gl::" + op, (a,))


@pytest.mark.parametrize("op", ["reduce128_nc", "reduce128", "reduce96_nc", "reduce96"])
def test_gl_reductions_on_every_word_combination(probe, op):
    """(hi, lo) over all 6^4 combinations of the edge words (the 96-bit forms: (hi32, lo) over 6^3), then random words"""
    k = 4 if op.startswith("reduce128") else 3
    hi, lo = word_cases(k)
    rng = np.random.default_rng(50 + GL[op])
    rh, rl = rand_any(rng, N_RANDOM), rand_any(rng, N_RANDOM)
    if k == 3:
        rh &= np.uint64(0xFFFFFFFF)
    hi, lo = np.concatenate([hi, rh]), np.concatenate([lo, rl])
    want = (obj(hi) * 2**64 + obj(lo)) % P
    check(probe.gl(GL[op], hi, lo), want, "gl::" + op, (hi, lo), exact=not op.endswith("_nc"))


def test_gl_inv_pow_root_of_unity(probe):
    """inv: canonical in, exact, inv(0) = 0.  pow: canonical base, any exponent (the edge lattice as exponents too).
    root_of_unity(k): exactly TWO_ADIC_ROOT^(2^(32 - k)), of order 2^k"""
    a = unary_cases(61, "canon", 1 << 16)
    got = obj(probe.gl(GL["inv"], a))
    A = obj(a)
    want = np.array([pow(int(x), P - 2, P) for x in A], dtype=object)
    check(got, want, "gl::inv", (a,))
    base, e = cross(EDGE_CANON, EDGE_ANY[::3])
    rng = np.random.default_rng(62)
    base, e = np.concatenate([base, rand_canon(rng, 4099)]), np.concatenate([e, rand_any(rng, 4099)])
    want = np.array([pow(int(x), int(y), P) for x, y in zip(base, e)], dtype=object)
    check(probe.gl(GL["pow"], base, e), want, "gl::pow", (base, e))
    k = u64(range(33))
    got = obj(probe.gl(GL["root"], k))
    root = 1753635133440165772
    want = np.array([pow(root, 1 << (32 - int(i)), P) for i in k], dtype=object)
    check(got, want, "gl::root_of_unity", (k,))
    for i in range(1, 33):
        assert pow(int(got[i]), 1 << (i - 1), P) == P - 1, i


def _e2_mul(a0, a1, b0, b1):
    return (a0 * b0 + 7 * a1 * b1) % P, (a0 * b1 + a1 * b0) % P


def _e2_pairs(seed, n_random):
    ed = [v for v in EDGE_CANON if v < 2**33 or v > P - 2**33 or v in (2**63, 2**63 - 1, 2**63 + 1)]
    e0, e1 = cross(ed, ed)
    rng = np.random.default_rng(seed)
    x0 = np.concatenate([e0, rand_canon(rng, n_random)])
    x1 = np.concatenate([e1, rand_canon(rng, n_random)])
    return np.stack([x0, x1], axis=1).ravel()


def test_gl_quadratic_extension(probe):
    """E2 = F_p[X]/(X^2 - 7): mul, sqr, inv (inv(0) = 0), pow, components canonical, exact"""
    x = _e2_pairs(70, 1 << 15)
    n = len(x) // 2
    y = np.roll(x.reshape(n, 2), 37, axis=0).ravel()
    X0, X1, Y0, Y1 = obj(x[0::2]), obj(x[1::2]), obj(y[0::2]), obj(y[1::2])

    def pair_check(got, w0, w1, what, ins):
        check(got[0::2], w0, what + " c0", ins)
        check(got[1::2], w1, what + " c1", ins)

    w0, w1 = _e2_mul(X0, X1, Y0, Y1)
    pair_check(probe.gl(GL["e2_mul"], x, y, width=2), w0, w1, "gl::E2 mul", (x[0::2], x[1::2], y[0::2], y[1::2]))
    w0, w1 = _e2_mul(X0, X1, X0, X1)
    pair_check(probe.gl(GL["e2_sqr"], x, width=2), w0, w1, "gl::E2 sqr", (x[0::2], x[1::2]))
    norm = (X0 * X0 - 7 * X1 * X1) % P
    ni = np.array([pow(int(v), P - 2, P) for v in norm], dtype=object)
    pair_check(probe.gl(GL["e2_inv"], x, width=2), (X0 * ni) % P, (-X1 * ni) % P, "gl::E2 inv", (x[0::2], x[1::2]))
    m = 2048 + 5
    xs, es = x[: 2 * m], rand_any(np.random.default_rng(71), m)
    es[: len(EDGE_ANY)] = u64(EDGE_ANY)                  # the edge lattice as exponents
    got = probe.gl(GL["e2_pow"], xs, c=es, width=2)
    for i in range(m):
        r, b, e = (1, 0), (int(xs[2 * i]), int(xs[2 * i + 1])), int(es[i])
        while e:
            if e & 1:
                r = _e2_mul(*r, *b)
            b = _e2_mul(*b, *b)
            e >>= 1
        assert (int(got[2 * i]), int(got[2 * i + 1])) == r, ("gl::E2 pow", i, _fmt(xs[2 * i: 2 * i + 2]), hex(int(es[i])))


# ---------------------------------------------------------------------------------------------------------------------------------
# gll:: (gl_lazy.hpp: carry chains through VCC and the hand-scheduled product blocks)

@pytest.mark.parametrize("op", ["canon", "add_nc", "sub_nc", "mul_nc"])
def test_gll_ops_on_the_edge_lattice(probe, op):
    """canon: any u64 in, exact.  add_nc / sub_nc: any u64 with a canonical w, congruent.  mul_nc: any u64 x any u64, congruent"""
    if op == "canon":
        a = unary_cases(80, "any")
        check(probe.gll(GLL[op], a), obj(a) % P, "gll::canon", (a,))
        return
    a, b = binary_cases(81 + GLL[op], "any", "any" if op == "mul_nc" else "canon")
    A, B = obj(a), obj(b)
    want = {"add_nc": (A + B) % P, "sub_nc": (A - B) % P, "mul_nc": (A * B) % P}[op]
    check(probe.gll(GLL[op], a, b), want, "gll::" + op, (a, b), exact=False)


@pytest.mark.parametrize("op", ["reduce128_nc", "reduce96_nc"])
def test_gll_reductions_on_every_word_combination(probe, op):
    k = 4 if op == "reduce128_nc" else 3
    hi, lo = word_cases(k)
    rng = np.random.default_rng(90 + k)
    rh, rl = rand_any(rng, N_RANDOM), rand_any(rng, N_RANDOM)
    if k == 3:
        rh &= np.uint64(0xFFFFFFFF)
    hi, lo = np.concatenate([hi, rh]), np.concatenate([lo, rl])
    check(probe.gll(GLL[op], hi, lo), (obj(hi) * 2**64 + obj(lo)) % P, "gll::" + op, (hi, lo), exact=False)


def test_gll_mul3_nc_keeps_its_three_chains_apart(probe):
    """three DIFFERENT operand pairs per lane (the edge cross product, rotated by a different amount for each chain): a swap of
    registers between the interleaved chains of the generated block gives some lane a product of the wrong pair"""
    a, b = binary_cases(95, "any", "any", n_random=(1 << 18) + 5)
    n = len(a)
    A3 = np.stack([a, np.roll(a, 1), np.roll(a, 3)], axis=1)
    B3 = np.stack([b, np.roll(b, 2), np.roll(b, 5)], axis=1)
    got = probe.gll(GLL["mul3_nc"], A3.ravel(), B3.ravel(), width=3).reshape(n, 3)
    for j in range(3):
        check(got[:, j], (obj(A3[:, j]) * obj(B3[:, j])) % P, "gll::mul3_nc chain %d" % j, (A3[:, j], B3[:, j]), exact=False)
    # the three products differ in (nearly) every lane, so a swap cannot hide behind equal values
    assert np.mean(got[:, 0] % np.uint64(P) != got[:, 1] % np.uint64(P)) > 0.9


# ---------------------------------------------------------------------------------------------------------------------------------
# lazy accumulators (gl.hpp Acc6 / Acc160, poseidon_pair.hpp acc6_reduce)

ALL_ONES = M64        # its 22 / 22 / 20-bit limbs are all ones


def _acc6_lanes(rng, terms, n):
    """start (lo, hi) per lane and x (values whose halves feed the products), y (the constants cut by limbs3) per term and lane.
    Lane classes: worst case (every half and every limb all ones, start all ones), edge words, random any u64"""
    start = np.zeros((n, 2), dtype=np.uint64)
    x, y = rand_any(rng, (terms, n)), rand_any(rng, (terms, n))
    start[:] = rand_any(rng, (n, 2)) & np.uint64(0xFFFFFFFF)
    w = n // 3
    x[:, :w], y[:, :w] = ALL_ONES, ALL_ONES
    start[:w] = 0xFFFFFFFF
    ew = u64(EDGE_ANY)
    x[:, w: 2 * w] = ew[rng.integers(0, len(ew), size=(terms, w))]
    y[:, w: 2 * w] = ew[rng.integers(0, len(ew), size=(terms, w))]
    start[w: 2 * w, 0] = u64(WORDS)[rng.integers(0, len(WORDS), size=w)]
    start[w: 2 * w, 1] = u64(WORDS)[rng.integers(0, len(WORDS), size=w)]
    start[1] = 0                                    # lane 1: the zero start
    return start.ravel(), x, y


@pytest.mark.parametrize("terms", [1, 2, 63, 64, 1023, 1024])
def test_acc6_filled_to_its_contract(probe, terms):
    """Acc6 claims 1024 products of (u32 half) x (22-bit limb) after set(lo, hi): filled with up to 1024 worst-case terms (halves and
    limbs all ones), edge words and random values, reduced by gl::Acc6::reduce and by poseidon_pair::acc6_reduce (the same sums,
    the hand-scheduled 128-bit reduction) -- congruent to start + sum x_t y_t"""
    rng = np.random.default_rng(100 + terms)
    n = 333
    start, x, y = _acc6_lanes(rng, terms, n)
    want = obj(start[0::2]) + obj(start[1::2]) * 2**32
    for t in range(terms):
        want = want + obj(x[t]) * obj(y[t])
    want = want % P
    for op, name in ((0, "gl::Acc6::reduce"), (1, "poseidon_pair::acc6_reduce")):
        check(probe.acc(op, start, x, y, terms), want, "%s after %d terms" % (name, terms), (start[0::2], start[1::2]), exact=False)


@pytest.mark.parametrize("terms", [1, 2, 64, 4099])
def test_acc160_far_past_its_carry_comment(probe, terms):
    """Acc160: up to 4099 maximal 64 x 64 products ((2^64 - 1)^2), so the carry word c reaches ~2^12 (the reduction's comment
    reasons with c < 2^5); plus edge words and random values -- congruent to the exact sum"""
    rng = np.random.default_rng(200 + terms)
    n = 257
    x, y = rand_any(rng, (terms, n)), rand_any(rng, (terms, n))
    w = n // 3
    x[:, :w], y[:, :w] = ALL_ONES, ALL_ONES
    ew = u64(EDGE_ANY)
    x[:, w: 2 * w] = ew[rng.integers(0, len(ew), size=(terms, w))]
    y[:, w: 2 * w] = ew[rng.integers(0, len(ew), size=(terms, w))]
    want = obj(np.zeros(n, dtype=np.uint64))
    for t in range(terms):
        want = want + obj(x[t]) * obj(y[t])
    got = probe.acc(2, np.zeros(2 * n, dtype=np.uint64), x, y, terms)
    check(got, want % P, "gl::Acc160 after %d terms" % terms, exact=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# BN254 Fq (fq.hpp): Montgomery form, R = 2^261, canonical values in and out

FP = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = pow(2, 261, FP)
RINV = pow(R, FP - 2, FP)


def fq_edges():
    v = [0, 1, 2, FP - 1, FP - 2, (FP - 1) // 2, (FP + 1) // 2, R, (R * R) % FP]
    v += [2**k for k in range(254) if 2**k < FP] + [FP - 2**k for k in range(254) if 2**k < FP]
    v += [(2**(29 * j) - 1) % FP for j in range(1, 10)]          # j 29-bit limbs all 0x1FFFFFFF (j = 9: the whole 261 bits)
    v += [(2**261 - 1) % FP, (2**256 - 1) % FP, (2**255 - 1) % FP, (2**254 - 1) % FP]
    return sorted(set(v))


def fq_pack(vals):
    """Python ints < 2^256 -> 4 u64 words each (little endian)"""
    return np.array([[(int(v) >> (64 * k)) & M64 for k in range(4)] for v in vals], dtype=np.uint64).ravel()


def fq_unpack(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    o = obj(w)
    return o[:, 0] + (o[:, 1] << 64) + (o[:, 2] << 128) + (o[:, 3] << 192)


def fq_random(rng, n):
    return [int.from_bytes(rng.bytes(32), "little") % FP for _ in range(n)]


def fq_check(got_words, want, what, ins):
    got = fq_unpack(got_words)
    bad = np.flatnonzero(np.asarray(got != np.asarray(want, dtype=object), dtype=bool))
    if len(bad):
        i = bad[0]
        raise AssertionError("%s: %d of %d wrong; first at %d: inputs %s -> got %s, want %s" % (
            what, len(bad), len(got), i, ", ".join(hex(int(x[i])) for x in ins), hex(int(got[i])), hex(int(want[i]))))


def _finv(v):
    return pow(int(v), FP - 2, FP)


@pytest.mark.parametrize("op", ["add", "sub", "mul"])
def test_fq_binary_ops(probe, op):
    """the edge values' full cross product plus 10^4 random pairs; mul is the Montgomery product a b 2^-261 mod p"""
    e = fq_edges()
    a, b = map(list, zip(*itertools.product(e, e)))
    rng = np.random.default_rng(300 + FQ[op])
    a += fq_random(rng, 10**4)
    b += fq_random(rng, 10**4)
    A, B = np.array(a, dtype=object), np.array(b, dtype=object)
    want = {"add": (A + B) % FP, "sub": (A - B) % FP, "mul": (A * B * RINV) % FP}[op]
    fq_check(probe.fq(FQ[op], fq_pack(a), fq_pack(b)), want, "fq::" + op, (A, B))


@pytest.mark.parametrize("op", ["neg", "dbl", "sqr", "to_mont", "from_mont", "inv", "inv_gcd", "is_zero"])
def test_fq_unary_ops(probe, op):
    """inv: Montgomery in / out (x R -> x^-1 R, i.e. R^2 / a for the stored a), inv(0) = 0; is_zero: 1 exactly for 0"""
    rng = np.random.default_rng(320 + FQ[op])
    a = fq_edges() + fq_random(rng, 10**4)
    A = np.array(a, dtype=object)
    if op in ("inv", "inv_gcd"):
        want = np.array([(R * R * _finv(v)) % FP if v else 0 for v in a], dtype=object)
    elif op == "is_zero":
        want = np.array([1 if v == 0 else 0 for v in a], dtype=object)
    else:
        want = {"neg": (-A) % FP, "dbl": (2 * A) % FP, "sqr": (A * A * RINV) % FP, "to_mont": (A * R) % FP,
                "from_mont": (A * RINV) % FP}[op]
    fq_check(probe.fq(FQ[op], fq_pack(a)), want, "fq::" + op, (A,))


def _fq2_cases(seed, n_random):
    e = [v for v in fq_edges() if v < 2**40 or v > FP - 2**40 or v in ((FP - 1) // 2, (FP + 1) // 2, R, (R * R) % FP)]
    rng = np.random.default_rng(seed)
    x0, x1 = map(list, zip(*itertools.product(e, e)))
    x0 += fq_random(rng, n_random)
    x1 += fq_random(rng, n_random)
    return np.array(x0, dtype=object), np.array(x1, dtype=object)


def _fq2_pack(c0, c1):
    return np.stack([fq_pack(c0).reshape(-1, 4), fq_pack(c1).reshape(-1, 4)], axis=1).ravel()


@pytest.mark.parametrize("op", ["fq2_add", "fq2_sub", "fq2_mul", "fq2_sqr", "fq2_inv", "fq2_inv_gcd"])
def test_fq2_ops(probe, op):
    """Fq2 = Fq[u]/(u^2 + 1) with Montgomery components: pairs of edge values plus random pairs; the second operand is the first
    list rotated"""
    x0, x1 = _fq2_cases(340 + FQ[op], 3000)
    y0, y1 = np.roll(x0, 101), np.roll(x1, 101)
    got = probe.fq(FQ[op], _fq2_pack(x0, x1), _fq2_pack(y0, y1), width=8).reshape(-1, 2, 4)
    if op == "fq2_add":
        w0, w1 = (x0 + y0) % FP, (x1 + y1) % FP
    elif op == "fq2_sub":
        w0, w1 = (x0 - y0) % FP, (x1 - y1) % FP
    elif op in ("fq2_mul", "fq2_sqr"):
        b0, b1 = (y0, y1) if op == "fq2_mul" else (x0, x1)
        w0, w1 = ((x0 * b0 - x1 * b1) * RINV) % FP, ((x0 * b1 + x1 * b0) * RINV) % FP
    else:
        norm = (x0 * x0 + x1 * x1) % FP
        ni = np.array([_finv(v) for v in norm], dtype=object)
        w0, w1 = (x0 * R * R * ni) % FP, (-x1 * R * R * ni) % FP
    fq_check(got[:, 0].ravel(), w0, "fq::" + op + " c0", (x0, x1, y0, y1))
    fq_check(got[:, 1].ravel(), w1, "fq::" + op + " c1", (x0, x1, y0, y1))


# ---------------------------------------------------------------------------------------------------------------------------------
# Poseidon layers (poseidon.hpp), one state per lane

def _gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_poseidon_header as g
    return g


@pytest.fixture(scope="module")
def poseidon_tables():
    g = _gen()
    rc = g.load_rc()
    first, _ = g.derive_fast_partial(rc)
    Mi, vs, ws = g.sparse_factor()
    return dict(rc=rc + [0] * 12, mds=g.mds_matrix(), dense=g.dense_matrices(first, Mi, vs, ws))


BYTE_WORDS = [0, M64, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F]


def layer_states(seed):
    """12-word states over ANY u64: every word all-0x00 / all-0xFF / all-0x80 / all-0x7F bytes, those patterns mixed per word and
    per byte, the Goldilocks edges, and random words (393 states: not a multiple of 64)"""
    rng = np.random.default_rng(seed)
    st = [[w] * 12 for w in BYTE_WORDS]
    st += [[BYTE_WORDS[(i + k) % 4] for i in range(12)] for k in range(4)]
    pats = np.array([0x00, 0xFF, 0x80, 0x7F], dtype=np.uint64)
    for _ in range(120):
        by = pats[rng.integers(0, 4, size=(12, 8))]
        st.append([int(sum(int(by[i, k]) << (8 * k) for k in range(8))) for i in range(12)])
    for _ in range(120):
        st.append([BYTE_WORDS[j] for j in rng.integers(0, 4, size=12)])
    ed = u64(EDGE_ANY)
    st += ed[rng.integers(0, len(ed), size=(60, 12))].tolist()
    st += rand_any(rng, (393 - len(st), 12)).tolist()
    return np.array(st, dtype=np.uint64)


def lane_isolation_states(rng, canonical):
    """64 waves in which 63 lanes hold state A and lane k holds state B (k = 0 .. 63), then one wave of 64 distinct states"""
    draw = rand_canon if canonical else rand_any
    A, B = draw(rng, 12), draw(rng, 12)
    waves = np.tile(A, (64, 64, 1))
    for k in range(64):
        waves[k, k] = B
    return np.concatenate([waves.reshape(-1, 12), draw(rng, (64, 12))])


def _matvec(rows, X, add=None):
    """exact (rows x 12 matrix) . state for every state of X (Python ints), + add[r] -> canonical"""
    Xo = obj(X)
    out = np.empty((Xo.shape[0], len(rows)), dtype=object)
    for r, row in enumerate(rows):
        acc = Xo[:, 0] * row[0]
        for e in range(1, 12):
            acc = acc + Xo[:, e] * row[e]
        out[:, r] = (acc + (add[r] if add is not None else 0)) % P
    return out


@pytest.mark.parametrize("mfma", [False, True])
def test_mds_full_layers(probe, poseidon_tables, mfma):
    """mds_full<ADD> / mds_full_mfma<ADD> against the exact circulant MDS (+ the added round constants): any u64 words, the byte-plane
    extremes of the matrix-pipe form's ^ 0x80 bias, and the lane-isolation waves -- congruent mod p"""
    X = np.concatenate([layer_states(400 + mfma), lane_isolation_states(np.random.default_rng(410 + mfma), False)])
    M = poseidon_tables["mds"]
    base = PSN["mds_mfma" if mfma else "mds"]
    check(probe.poseidon(base, X).ravel(), _matvec(M, X).ravel(), ("mds_full_mfma" if mfma else "mds_full") + "<false>", exact=False)
    for rnd in (1, 17, 29, 30):
        add = poseidon_tables["rc"][12 * rnd: 12 * rnd + 12]
        got = probe.poseidon(base + 1, X, arg=rnd)
        for r in range(12):
            check(got[:, r], _matvec([M[r]], X, [add[r]])[:, 0], "%s<true> round %d row %d" % ("mds_full_mfma" if mfma else "mds_full", rnd, r),
                  (X[:, r],), exact=False)


def test_dense_mfma_every_matrix(probe, poseidon_tables):
    """every dense_mfma matrix (the merged layer of full round 3; W and V of both lazy blocks) with and without a per-lane addend,
    against the exact matrices of tools/gen_poseidon_header.py::dense_matrices (not the *_model functions, which mirror the kernel)"""
    mats = poseidon_tables["dense"]
    assert len(mats) == probe.dense_mats
    X = np.concatenate([layer_states(420), lane_isolation_states(np.random.default_rng(421), False)])
    addend = rand_any(np.random.default_rng(422), (X.shape[0], 11))
    addend[:8] = M64
    addend[8:16] = 0
    addend[16:24] = 0x8080808080808080
    for mi, (Mx, add) in enumerate(mats):
        want = _matvec(Mx, X, add)
        got = probe.poseidon(PSN["dense"], X, arg=mi)
        check(got[:, :11].ravel(), want.ravel(), "dense_mfma<false> matrix %d" % mi, exact=False)
        got = probe.poseidon(PSN["dense_addend"], X, arg=mi, addend=addend)
        check(got[:, :11].ravel(), ((want + obj(addend)) % P).ravel(), "dense_mfma<true> matrix %d" % mi, exact=False)


def permute_states():
    from tests.test_oracle_generic import KAT
    st = [k[0] for k in KAT] + [[0] * 12, [P - 1] * 12]
    for i in range(12):
        s = [0] * 12
        s[i] = P - 1
        st.append(s)
    st += [[2**32 - 1] * 12, [2**32] * 12, [(2**32 - 1) if i % 2 else 2**32 for i in range(12)], [P - 2**32] * 12,
           [0xFFFFFFFF00000000] * 12, [2**63] * 12]
    rng = np.random.default_rng(430)
    ed = u64(EDGE_CANON)
    st += ed[rng.integers(0, len(ed), size=(64, 12))].tolist()
    st += rand_canon(rng, (200, 12)).tolist()
    return np.array(st, dtype=np.uint64)


@pytest.mark.parametrize("mfma", [False, True])
def test_permute_known_answers_edges_and_lane_isolation(probe, mfma):
    """permute<false> (VALU linear layers) and permute<true> (the matrix-pipe form every leaf hash uses) on the three KATs, all 0,
    all p - 1, one word p - 1, the 2^32 - 1 / 2^32 patterns, random states, and the lane-isolation waves: every lane equals
    _oracle.permute of its own state"""
    from tests.test_oracle_generic import KAT
    X = np.concatenate([permute_states(), lane_isolation_states(np.random.default_rng(440), True)])
    got = probe.poseidon(PSN["permute_mfma" if mfma else "permute"], X)
    for i, (_, out) in enumerate(KAT):
        assert [int(v) for v in got[i]] == out, ("KAT", i)
    memo = {}
    for i in range(X.shape[0]):
        key = X[i].tobytes()
        if key not in memo:
            memo[key] = _oracle.permute(X[i])
        assert (got[i] == memo[key]).all(), ("permute<%s>" % ("true" if mfma else "false"), i, _fmt(X[i]))


# ---------------------------------------------------------------------------------------------------------------------------------
# structured columns through the product ABI: every leaf route, the three LDE paths, the NTT

def structured_columns(ncols, n):
    """column c cycles through: all 0, all p - 1, every cell p - 1 - c, an impulse (1 in one row), alternating 0 / p - 1, and
    words with all-ones halves (2^32 - 1 and p - 1 = 0xFFFFFFFF00000000, alternating)"""
    cols = np.zeros((ncols, n), dtype=np.uint64)
    for c in range(ncols):
        k = c % 6
        if k == 1:
            cols[c] = P - 1
        elif k == 2:
            cols[c] = P - 1 - c
        elif k == 3:
            cols[c, (7 * c + 3) % n] = 1
        elif k == 4:
            cols[c, 1::2] = P - 1
        elif k == 5:
            cols[c, 0::2], cols[c, 1::2] = 0xFFFFFFFF, 0xFFFFFFFF00000000
    return cols


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=2 << 30)
    yield c
    c.close()


LEAF_NAMES = ("poseidon_leaves", "poseidon_leaves_pair", "poseidon_leaves_noop")


@pytest.mark.parametrize("log_leaves,ncols,route", [(17, 8, "poseidon_leaves"), (17, 13, "poseidon_leaves"),
                                                    (5, 5, "poseidon_leaves_pair"), (10, 12, "poseidon_leaves_pair"),
                                                    (16, 7, "poseidon_leaves_pair"), (6, 4, "poseidon_leaves_noop"),
                                                    (17, 3, "poseidon_leaves_noop")])
def test_leaf_routes_on_structured_columns(ctx, log_leaves, ncols, route):
    """sipp_poseidon_leaves on structured columns, on each of its three routes -- one state per lane (more than 2^16 leaves), two
    lanes per state (32 .. 2^16 leaves, more than 4 columns), the unhashed copy (4 columns or fewer) -- leaf by leaf against the
    oracle; the profile names the route, so that a routing change cannot silently retarget the case"""
    from sipp_amd._lib import to_device, to_host
    n = 1 << log_leaves
    cells = structured_columns(ncols, n)
    ctx.profile(True)
    ctx.profile_reset()
    dig = to_host(ctx.poseidon_leaves(to_device(cells), log_leaves))
    rep = ctx.profile_report()
    ctx.profile(False)
    assert route in rep and not any(k in rep for k in LEAF_NAMES if k != route), (route, sorted(rep))
    rows = sorted(set(range(0, min(n, 70))) | set(range(max(0, n - 70), n)) | set(range(0, n, max(1, n // 509))) |
                  {(7 * c + 3) % n for c in range(ncols)})
    for j in rows:
        # hash_or_noop: four columns or fewer are the digest itself, zero-padded
        want = np.concatenate([cells[:, j], np.zeros(4 - ncols, dtype=np.uint64)]) if ncols <= 4 else _oracle.hash_no_pad(cells[:, j])
        assert (dig[j] == want).all(), (route, log_leaves, ncols, j)


@pytest.mark.parametrize("log_n,ncols", [(6, 7), (9, 6), (12, 6), (14, 7), (15, 6), (17, 6)])
def test_commit_paths_on_structured_columns(ctx, log_n, ncols):
    """PolynomialBatch::from_values on structured columns through the pass-by-pass path (below 2^10), the whole-column kernel
    (2^10 .. 2^14) and the tree-of-rings sweeps (2^15 and above): coefficients, every LDE cell, every tree level and the cap
    equal the oracle's"""
    from sipp_amd._lib import to_device, to_host
    vals = structured_columns(ncols, 1 << log_n)
    ref = _oracle.Batch(vals, log_n)
    coeffs, lde, tree, cap = ctx.commit(to_device(vals), log_n)
    assert (to_host(coeffs) == ref.coeffs).all()
    assert (to_host(lde).T == ref.leaves).all()
    m = 2 << log_n
    t = to_host(tree)
    off = 0
    for lvl in range(log_n + 1 - 4 + 1):
        cnt = m >> lvl
        assert (t[off:off + cnt] == ref.level(lvl)).all(), lvl
        off += cnt
    assert (cap == ref.cap).all()


@pytest.mark.parametrize("log_n", [4, 5, 8, 12, 13, 14, 17, 20])
def test_ntt_on_structured_columns(ctx, oracle, log_n):
    """the NTT forward and inverse on structured columns at the sizes of test_gpu_generic.py::test_ntt_matches_oracle (without 2^22)"""
    from sipp_amd._lib import to_device, to_host
    a = structured_columns(6, 1 << log_n)
    d = to_device(a)
    got = to_host(ctx.ntt(d, log_n))
    for c in range(a.shape[0]):
        ref = a[c].copy()
        oracle.orc_fft(ref, log_n)
        assert (got[c] == ref).all(), (log_n, c)
    back = to_host(ctx.ntt(d, log_n, inverse=True))
    assert (back == a).all(), log_n
