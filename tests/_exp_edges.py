"""The edge catalogue of the five exponentiation AIRs (G1 / G2 / Fq12, kinds 0 / 1 / 2, and the hardened G1 / G2 kinds 4 / 5): named IO
records (x, offset, exponent) with the output computed here, in Python integers (oracle/py/bn254.py): out = offset + [e] x for the
curves, out = offset * x^e for Fq12.  Shared by tests/test_oracle_exp_edges.py (the oracle against integers), tests/test_gpu_exp_edges.py
(the device against the oracle) and scripts/stress_parity.py.  Deterministic: no RNG, every search walks from a fixed start.

What the records are chosen for (sipp_amd/csrc/trace.hip):
  * operands whose 16-bit limbs are all near 0xFFFF, 0 or a single set bit (the gadget rows: sign, quotient limbs, carries);
  * exponents at the 32-bit word boundaries and >= r (the closed-form remaining-exponent cells);
  * Fq12 zero / one / maximal coefficients (the MyFq12 product and the tower conversion; columns constant over a whole trace);
  * pairs of points whose x coordinates differ in one limb only, by a few units, in both orders (the hardened kinds' search for the
    first differing limb and its Goldilocks inverse of a positive / negative difference);
  * chords of a prescribed slope (1, ~sqrt(2p)): rows whose gadget identity holds over the INTEGERS (all 17 quotient limbs zero);
  * `refused`: records one or both AIR variants have no witness for.
"""
import functools
from collections import namedtuple
from math import isqrt

from oracle.py import bn254 as bn
from oracle.py import sipp_native as sn

P, R = bn.P, bn.R
TOP = (0x3063 << 240) + (1 << 240) - 1          # the largest value below p whose 15 low limbs are all 0xFFFF
assert TOP < P and TOP + (1 << 240) > P
FIELD_VALUES = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, TOP, 1 << 240, (1 << 128) - 1, 1 << 16, (1 << 16) - 1]

EXPONENTS = [0, 1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, 1 << 64, 1 << 224, 1 << 255, (1 << 255) + 1, (1 << 256) - 1,
             R - 1, R, R + 1, int("AA" * 32, 16), int("55" * 32, 16), int("FFFFFFFF00000000" * 4, 16)]
EDGE_SCALARS = EXPONENTS                        # (the name scripts/stress_parity.py uses)

Rec = namedtuple("Rec", "name x off e out")
# plain / hardened: True where that AIR variant has NO witness for the record (for Fq12 only `plain` is meaningful); `out` is the claimed
# output (the true one where a variant proves the record)
Refused = namedtuple("Refused", "name x off e out plain hardened")

WORDS = {0: 56, 1: 104, 2: 296}
OUT_WORDS = {0: 16, 1: 32, 2: 96}


def base_kind(kind):
    return kind - 4 if kind >= 4 else kind


# ---------------- points ----------------
def g1_y(x):
    rhs = (x * x * x + 3) % P
    y = pow(rhs, (P + 1) // 4, P)
    return y if y * y % P == rhs else None


def g1_walk(x0, step):
    """the first point of E(Fp) on x0, x0 + step, ...; every point is legal (cofactor 1)"""
    x = x0 % P
    while True:
        y = g1_y(x)
        if y is not None:
            return (x, y)
        x = (x + step) % P


def g2_y(x):
    return bn.f2_sqrt(bn.f2_add(bn.f2_mul(bn.f2_mul(x, x), x), bn.B2))


def g2_walk(c0, c1, step, on_c1=False):
    """the first point of E'(Fp2) walking x.c0 (or x.c1) by `step`; the G2 exponentiation AIR asks for the curve, not the subgroup"""
    while True:
        y = g2_y((c0, c1))
        if y is not None:
            return ((c0, c1), y)
        if on_c1:
            c1 = (c1 + step) % P
        else:
            c0 = (c0 + step) % P


@functools.lru_cache(None)
def g1_points():
    starts = ((P - 1, -1), (TOP, -1), (0, 1), (1 << 240, 1 << 240), ((1 << 128) - 1, 1 << 128))
    return [("near_pm1", "near_top", "near_0", "near_2p240", "near_2p128_m1")[i] for i in range(5)], [g1_walk(a, s) for a, s in starts]


@functools.lru_cache(None)
def g2_points():
    starts = ((P - 1, P - 1, -1), (TOP, TOP, -1), (0, 1, 1), (1, 0, 1), (1 << 240, 0, 1 << 240))
    return [("near_pm1", "near_top", "near_0_1", "near_1_0", "near_2p240")[i] for i in range(5)], [g2_walk(a, b, s) for a, b, s in starts]


@functools.lru_cache(None)
def g1_limb_pairs():
    """[(name, A, B, limb)]: A.x and B.x equal in every 16-bit limb but `limb`, where B's is A's + k for the first k >= 1 that is on the curve"""
    out = []
    for limb, start, step in ((0, (1 << 200) + 0x1234, 1 << 16), (15, (0x1000 << 240) + 5, 1)):
        A = g1_walk(start, step)
        k = 1
        while g1_y(A[0] + (k << (16 * limb))) is None:
            k += 1
        B = (A[0] + (k << (16 * limb)), g1_y(A[0] + (k << (16 * limb))))
        assert (A[0] >> (16 * limb)) & 0xFFFF < 0xFFFF - k and B[0] < P
        out.append(("limb%d" % limb, A, B, limb))
    return out


@functools.lru_cache(None)
def g2_limb_pairs():
    """limb 0 of x.c0 and limb 15 of x.c1 (limb 31 of the 32 the hardened AIR compares)"""
    out = []
    for limb, c0, c1, on_c1 in ((0, (1 << 200) + 0x1234, 7, True), (31, 9, (0x1000 << 240) + 5, False)):
        A = g2_walk(c0, c1, 1, on_c1=on_c1)
        k = 1
        while True:
            d = k << (16 * (limb % 16))
            xb = (A[0][0] + d, A[0][1]) if limb < 16 else (A[0][0], A[0][1] + d)
            y = g2_y(xb)
            if y is not None:
                break
            k += 1
        assert max(xb) < P and k < 0x1000
        out.append(("limb%d" % limb, A, (xb, y), limb))
    return out


# ---------------- chords of a prescribed slope: gadget identities that hold over the integers ----------------
class _F1:
    b = 3
    zero = 0
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    half = staticmethod(lambda a: a * ((P + 1) // 2) % P)
    comps = staticmethod(lambda a: (a,))

    @staticmethod
    def sqrt(a):
        y = pow(a, (P + 1) // 4, P)
        return y if y * y % P == a else None


class _F2:
    b = bn.B2
    zero = (0, 0)
    add = staticmethod(bn.f2_add)
    sub = staticmethod(bn.f2_sub)
    mul = staticmethod(bn.f2_mul)
    half = staticmethod(lambda a: bn.f2_scal(a, (P + 1) // 2))
    comps = staticmethod(lambda a: a)
    sqrt = staticmethod(bn.f2_sqrt)


def chord_with_slope(F, Pt, lam):
    """a second point R of the curve on the line of slope `lam` through Pt (None if the line meets the curve nowhere else over the field):
    x^3 + b = (lam (x - xP) + yP)^2 has the roots xP, xR, xT with xR + xT = lam^2 - xP and xP xR + xP xT + xR xT = -2 lam c"""
    xp, yp = Pt
    c = F.sub(yp, F.mul(lam, xp))
    s = F.sub(F.mul(lam, lam), xp)
    m = F.sub(F.sub(F.zero, F.mul(F.add(lam, lam), c)), F.mul(xp, s))
    root = F.sqrt(F.sub(F.mul(s, s), F.add(F.add(m, m), F.add(m, m))))
    if root is None:
        return None
    xr = F.half(F.add(s, root))
    if xr == xp:
        return None
    return (xr, F.add(F.mul(lam, xr), c))


def _imul(a, b):
    """the integer (unreduced) product of two tuples of Fq components"""
    if len(a) == 1:
        return (a[0] * b[0],)
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def chord_row_E(F, Pt, Rt, lam):
    """the integer values E of the slope / x3 / y3 gadgets (per Fq component) on the add row R + P with slope lam: 0 = all 17 quotient limbs zero"""
    x3 = F.sub(F.sub(F.mul(lam, lam), Rt[0]), Pt[0])
    y3 = F.sub(F.mul(lam, F.sub(Rt[0], x3)), Rt[1])
    L, xr, yr, xp, yp, x3, y3 = (F.comps(v) for v in (lam, Rt[0], Rt[1], Pt[0], Pt[1], x3, y3))
    sub = lambda a, b: tuple(u - v for u, v in zip(a, b))
    s, x, y = _imul(L, sub(xp, xr)), _imul(L, L), _imul(L, sub(xr, x3))
    E = {}
    for k in range(len(L)):
        E["slope%d" % k] = s[k] - (yp[k] - yr[k])
        E["x3%d" % k] = x[k] - xr[k] - xp[k] - x3[k]
        E["y3%d" % k] = y[k] - yr[k] - y3[k]
    return E


@functools.lru_cache(None)
def zero_quotient_chords(kind):
    """[(name, P, R, gadgets)]: records x = P, offset = R, e = 1 whose first row has E = 0 over the integers for the named gadgets; found by
    walking P from a fixed start until every slope / x3 / y3 gadget of the AIR is covered"""
    if kind == 0:
        F, slopes = _F1, [("unit", 1), ("sqrt2p", isqrt(2 * P))]
        pt = lambda i: g1_walk((1 << 250) + i, 1)
        need = {"slope0", "x30", "y30"}
    else:
        F, slopes = _F2, [("unit", (1, 0)), ("sqrt2p", (isqrt(2 * P), 0)), ("sqrtp_sqrtp", (isqrt(P), isqrt(P)))]
        pt = lambda i: g2_walk((1 << 250) + i, 1 << 249, 1)
        need = {"slope0", "slope1", "x30", "x31", "y30", "y31"}
    out, i = [], 0
    while need:
        Pt = pt(i)
        i = (Pt[0] if kind == 0 else Pt[0][0]) - (1 << 250) + 1
        for sname, lam in slopes:
            Rt = chord_with_slope(F, Pt, lam)
            if Rt is None:
                continue
            hit = {g for g, v in chord_row_E(F, Pt, Rt, lam).items() if v == 0} & need
            if hit:
                need -= hit
                out.append(("chord_%s_%d" % (sname, len(out)), Pt, Rt, tuple(sorted(hit))))
        assert i < 4096, "the walk for integer chords did not end"
    return out


# ---------------- Fq12 elements (MyFq12 coefficients c_0 .. c_11) ----------------
F12_ELEMENTS = [
    ("zero", [0] * 12),
    ("one", [1] + [0] * 11),
    ("all_pm1", [P - 1] * 12),
    ("all_top", [TOP] * 12),
    ("w6", [0] * 6 + [1] + [0] * 5),
    ("alt_pm1_0", [P - 1, 0] * 6),
    ("c11_pm1", [0] * 11 + [P - 1]),
    ("all_2p240", [1 << 240] * 12),
    ("base_field", [(P + 1) // 2] + [0] * 11),
    ("field_values", list(FIELD_VALUES)),
]
F12_SPECIAL = [e for _, e in F12_ELEMENTS[:5]] + [[P - 1] + [0] * 11]      # (what scripts/stress_parity.py mixes into its random elements)


# ---------------- group law / power with the identity as None ----------------
def g_out(kind, x, off, e):
    if kind == 0:
        return bn.g1_add(off, bn.g1_mul(x, e))
    if kind == 1:
        return bn.g2_add(off, bn.g2_mul(x, e))
    return bn.f12_mul(off, bn.f12_pow(x, e))


def _cycle(names, vals, kind):
    """record i pairs value i with a later one as its offset and takes the next exponent: every exponent once, every value at least once.
    The curves' cycle leaves out the exponents 1 and 3: the limb-distance pairs carry them"""
    exps = [(j, e) for j, e in enumerate(EXPONENTS) if kind == 2 or e not in (1, 3)]
    n, recs = len(vals), []
    for i in range(30 if kind == 2 else len(exps)):
        a, b = i % n, (i + 1 + i // n) % n
        j, e = exps[i % len(exps)]
        assert a != b
        recs.append(Rec("%s__%s__e%d" % (names[a], names[b], j), vals[a], vals[b], e, g_out(kind, vals[a], vals[b], e)))
    return recs


@functools.lru_cache(None)
def records(kind):
    """the records every variant of the kind's AIR proves (kind 0 G1, 1 G2, 2 Fq12; 4 / 5: the same lists as 0 / 1)"""
    kind = base_kind(kind)
    if kind == 2:
        recs = _cycle([n for n, _ in F12_ELEMENTS], [v for _, v in F12_ELEMENTS], 2)
        zero, pm1 = F12_ELEMENTS[0][1], F12_ELEMENTS[2][1]
        recs.append(Rec("zero_zero_0", zero, zero, 0, g_out(2, zero, zero, 0)))
        recs.append(Rec("pm1_pm1_max", pm1, pm1, (1 << 256) - 1, g_out(2, pm1, pm1, (1 << 256) - 1)))
        return recs
    names, pts = g1_points() if kind == 0 else g2_points()
    recs = _cycle(names, pts, kind)
    for name, A, B, _ in (g1_limb_pairs() if kind == 0 else g2_limb_pairs()):
        for e in (1, 3):
            recs.append(Rec("%s_pos_e%d" % (name, e), B, A, e, g_out(kind, B, A, e)))     # P.x - R.x = +k in the limb
            recs.append(Rec("%s_neg_e%d" % (name, e), A, B, e, g_out(kind, A, B, e)))     # ... = -k
    for name, Pt, Rt, _ in zero_quotient_chords(kind):
        recs.append(Rec(name, Pt, Rt, 1, g_out(kind, Pt, Rt, 1)))
    assert all(r.out is not None for r in recs)
    return recs


@functools.lru_cache(None)
def limb_pair_records(kind):
    return [r for r in records(kind) if r.name.startswith("limb")]


@functools.lru_cache(None)
def refused(kind):
    kind = base_kind(kind)
    if kind == 2:
        a, b = F12_ELEMENTS[3][1], F12_ELEMENTS[7][1]
        out = g_out(2, a, b, 3)
        return [Refused("wrong_output", a, b, 3, [out[0] ^ 1] + out[1:], True, True)]
    neg = bn.g1_neg if kind == 0 else bn.g2_neg
    mul = bn.g1_mul if kind == 0 else bn.g2_mul
    _, pts = g1_points() if kind == 0 else g2_points()
    A, B, C_ = pts[0], pts[1], pts[3]
    bump = (lambda p: (p[0], (p[1] + 1) % P)) if kind == 0 else (lambda p: (p[0], ((p[1][0] + 1) % P, p[1][1])))
    out = g_out(kind, A, B, 5)
    flip = (out[0] ^ 1, out[1]) if kind == 0 else ((out[0][0] ^ 1, out[0][1]), out[1])
    e255 = (1 << 255) + 1
    return [
        Refused("x_off_curve", bump(A), B, 5, out, True, True),
        Refused("offset_off_curve", A, bump(B), 5, out, True, True),
        Refused("wrong_output", A, B, 5, flip, True, True),
        # the first addition is R + P with R = P: the plain chord rule has no slope, the hardened AIR takes the next row's double
        Refused("x_is_offset_e3", A, A, 3, mul(A, 4), True, False),
        Refused("x_is_offset_e3_top", B, B, 3, mul(B, 4), True, False),
        # R = -P on a used addition: the accumulator passes through the identity (hardened only)
        Refused("offset_is_minus_x_e3", A, neg(A), 3, mul(A, 2), True, False),
        Refused("offset_is_minus_x_e3_top", B, neg(B), 3, mul(B, 2), True, False),
        # the OUTPUT is the identity: no affine record says it
        Refused("output_identity_e5", C_, neg(mul(C_, 5)), 5, C_, True, True),
        Refused("output_identity_e1", A, neg(A), 1, A, True, True),
        # R = P on the LAST add row (bit 255 set): no row is left to hand the double over
        Refused("meets_power_on_last_add_row", C_, mul(C_, (1 << 255) - 1), e255, mul(C_, 1 << 256), True, True),
    ]


# ---------------- words ----------------
def _val_words(kind, v):
    return (bn.g1_to_u32, bn.g2_to_u32, bn.f12_to_u32)[base_kind(kind)](v)


def rec_words(kind, r, blank=False):
    """one record in the C-ABI layout (x, offset, exp_val, output); blank: the output words zeroed"""
    k = base_kind(kind)
    out = [0] * OUT_WORDS[k] if blank else _val_words(k, r.out)
    return _val_words(k, r.x) + _val_words(k, r.off) + sn.exp_to_u32(r.e) + out


def words(kind, recs, blank=False):
    return [rec_words(kind, r, blank) for r in recs]
