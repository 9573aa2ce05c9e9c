"""The edge catalogue of the pairing products (sipp_inner_product(s): miller_kernel, product_kernel, final_exp_kernel of
sipp_amd/csrc/pairing.hip) and of the native chain's host arithmetic (sipp_amd/csrc/native.hip): named calls -- `count` groups of pairs
(A_i, B_i), None = the point at infinity -- with the 12 MyFq12 coefficients every group must give, computed here in Python integers
(oracle/py/bn254.py).  Shared by tests/test_oracle_pairing_cases.py (the catalogue against itself and the C reading of the pairing),
tests/test_gpu_pairing_edges.py (the device against the catalogue, word for word) and scripts/stress_native.py.  Deterministic: no RNG.

Two kinds of expectation:
  * small groups (at most 8 pairs): bn.multi_pairing -- Miller loops and the plain power, pair by pair;
  * size cases (255 .. 513 pairs, the strided partial products and the tree of product_kernel, group offsets that are no multiple of
    256): the points are A_i = [a_0 + i da] G1, B_i = [b_0 + i db] G2, built by repeated ADDITION, and the product is the closed form
    e(G1, G2)^(sum a_i b_i mod r) -- one pairing and one power, independent of the device (test_oracle_pairing_cases.py holds the closed
    form against multi_pairing at n = 8).

What the points are chosen for: G1 coordinates next to 0, p - 1, the largest value with fifteen 0xFFFF limbs, 2^240 and 2^128 - 1
(tests/_exp_edges.g1_points(): every point of E(Fp) is legal, the cofactor is 1), -G1 = (1, p - 2), scalars next to 0 and r, the three
infinity shapes of miller_kernel (A only, B only, both) at the first and the last place of a group and alone, groups whose product is
exactly ONE, groups of which a single pair is finite (a dropped stride or tree slot shows directly).

G2 coordinates: edge coordinates cannot be aimed at inside the r-torsion of the twist (its points are found by scalar multiplication,
not by walking x), and the products' contract asks for points of G2 -- so the catalogue holds NO twist point outside the subgroup; the
G2 side varies by scalar (1, 2, r - 1, r - 2, (r + 1) / 2, small multiples) only.

Messages for the verifier: `crafted_proofs()` puts the Fq12 edge elements of tests/_exp_edges.py (all coefficients p - 1, all at TOP,
w^6, a lone c11 = p - 1, ...) in place of Z, Z_L, Z_R behind honest A, B -- what the Montgomery product f12_mul_host and the running
product Z Z_L^x Z_R^(1/x) never see from an honest prover; `tampered_proofs()` is the table of single-bit changes to an honest proof.
"""
import functools
import os
from collections import namedtuple

import numpy as np

from oracle.py import bn254 as bn
from oracle.py import sipp_native as sn
from tests import _exp_edges as E

P, R = bn.P, bn.R
G1, G2 = bn.G1, bn.G2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# one call of sipp_inner_products: len(groups) = count groups of equally many pairs; want[k] = the 12 coefficients of group k
Case = namedtuple("Case", "name groups want")

SIZES = (255, 256, 257, 511, 512, 513)
INF_SHAPES = ("g1", "g2", "both")


# ---------------- words ----------------
def g1_words(p):
    return [0] * 16 if p is None else bn.g1_to_u32(p)


def g2_words(q):
    return [0] * 32 if q is None else bn.g2_to_u32(q)


def case_words(case):
    """(g1 [count n, 16], g2 [count n, 32], count, want [count, 96]) of one call"""
    pairs = [pq for g in case.groups for pq in g]
    assert len({len(g) for g in case.groups}) == 1
    return (np.array([g1_words(a) for a, _ in pairs], dtype=np.uint32), np.array([g2_words(b) for _, b in pairs], dtype=np.uint32),
            len(case.groups), np.array([bn.f12_to_u32(w) for w in case.want], dtype=np.uint32))


def infinity(shape, a, b):
    """the pair (a, b) with infinity in place of a, of b or of both: the side that stays is a real point the kernel has to ignore"""
    return {"g1": (None, b), "g2": (a, None), "both": (None, None)}[shape]


# ---------------- exact small groups ----------------
@functools.lru_cache(None)
def _multi(group):
    return bn.multi_pairing([a for a, _ in group], [b for _, b in group])


def exact(name, groups):
    groups = [tuple(g) for g in groups]
    return Case(name, groups, [_multi(g) for g in groups])


@functools.lru_cache(None)
def single_pairs():
    """[(name, A, B)]: the finite single pairs (also what the C reading orc_pairing is held against)"""
    out = [("g1_g2", G1, G2), ("negg1_g2", bn.g1_neg(G1), G2), ("g1_negg2", G1, bn.g2_neg(G2))]
    for name, s in (("1", 1), ("2", 2), ("rm1", R - 1), ("rm2", R - 2), ("half", (R + 1) // 2)):
        out.append(("s%s_on_g1" % name, bn.g1_mul(G1, s), G2))
        if s != 1:
            out.append(("s%s_on_g2" % name, G1, bn.g2_mul(G2, s)))
    names, pts = E.g1_points()
    G2x3 = bn.g2_mul(G2, 3)
    for name, pt in zip(names, pts):
        out.append(("%s_g2" % name, pt, G2))
        out.append(("%s_3g2" % name, pt, G2x3))
    return out


@functools.lru_cache(None)
def small_groups():
    """[(name, groups)]: the calls of at most 8 pairs per group, without their expectations (points only: cheap)"""
    cases = [(name, [[(a, b)]]) for name, a, b in single_pairs()]
    _, pts = E.g1_points()
    # infinity in a group of 3, first and last place
    f0, f1 = (bn.g1_mul(G1, 2), G2), (pts[0], bn.g2_mul(G2, 3))
    spare = (bn.g1_mul(G1, 5), bn.g2_mul(G2, 5))
    for shape in INF_SHAPES:
        inf = infinity(shape, *spare)
        cases.append(("inf_%s_first_of_3" % shape, [[inf, f0, f1]]))
        cases.append(("inf_%s_last_of_3" % shape, [[f0, f1, inf]]))
        cases.append(("only_inf_%s_n1" % shape, [[inf]]))
    cases.append(("only_inf_n3", [[infinity(s, *spare) for s in INF_SHAPES]]))
    # cancelling groups (the expectation is computed, test_oracle_pairing_cases.py asserts that it is ONE)
    Pt, Q, a = pts[0], bn.g2_mul(G2, 7), 0x1234567
    cases.append(("cancel_negp", [[(Pt, Q), (bn.g1_neg(Pt), Q)]]))
    cases.append(("cancel_negq", [[(Pt, Q), (Pt, bn.g2_neg(Q))]]))
    cases.append(("cancel_scalar", [[(bn.g1_mul(Pt, a), Q), (Pt, bn.g2_mul(Q, R - a))]]))
    # one pair k times
    cases.append(("repeat_4", [[(pts[1], bn.g2_mul(G2, 2))] * 4]))
    # ragged tree levels
    A, B, _, _ = chain()
    for n in (3, 5, 6, 7):
        cases.append(("ragged_n%d" % n, [list(zip(A[:n], B[:n]))]))
    # seven groups of one pair: every value different
    seven = [single_pairs()[i] for i in (0, 1, 4, 8, 10, 12, 15)]
    cases.append(("count7_n1", [[(a, b)] for _, a, b in seven]))
    return [(name, [tuple(g) for g in groups]) for name, groups in cases]


@functools.lru_cache(None)
def small_cases():
    """the small calls with bn.multi_pairing's expectation for every group (about 45 final exponentiations in Python integers: what
    the CPU test computes; the GPU test reads the same values from SMALL_RECORDED)"""
    cases = [exact(name, groups) for name, groups in small_groups()]
    assert len({tuple(w) for w in cases[-1].want}) == 7
    return cases


SMALL_RECORDED = os.path.join(GOLDEN, "pairing_small_cases.npz")


def small_cases_recorded():
    """small_cases() with the expectations read from tests/golden/pairing_small_cases.npz (name -> [count, 96] words), which
    tests/test_oracle_pairing_cases.py holds against small_cases() value for value; written by `python -m tests._pairing_cases`"""
    d = np.load(SMALL_RECORDED)
    assert sorted(d.files) == sorted(name for name, _ in small_groups())
    return [Case(name, groups, [f12_of([int(x) for x in row]) for row in d[name]]) for name, groups in small_groups()]


# ---------------- size cases: closed form ----------------
A0, DA = 0x1234567890ABCDEF1234567890ABCDEF1234567, 0x0FEDCBA9876543210FEDCBA9876543210FEDCBA987654321
B0, DB = 0x7E57AB1E5CA1AB1E7E57AB1E5CA1AB1E, 0x123456789ABCDEF0123456789ABCDEF0123456789ABCDEF
CHAIN_LEN = 5 * 257


@functools.lru_cache(None)
def chain():
    """(A, B, a, b): A_i = [a_i] G1, B_i = [b_i] G2 with a_i = A0 + i DA, b_i = B0 + i DB (mod r), every point from the one before by
    ONE addition"""
    da, db = bn.g1_mul(G1, DA), bn.g2_mul(G2, DB)
    A, B = [bn.g1_mul(G1, A0)], [bn.g2_mul(G2, B0)]
    for _ in range(CHAIN_LEN - 1):
        A.append(bn.g1_add(A[-1], da))
        B.append(bn.g2_add(B[-1], db))
    assert None not in A and None not in B
    return A, B, [(A0 + i * DA) % R for i in range(CHAIN_LEN)], [(B0 + i * DB) % R for i in range(CHAIN_LEN)]


@functools.lru_cache(None)
def e_generators():
    return bn.pairing(G1, G2)


def closed_form(s):
    """e(G1, G2)^s"""
    return bn.f12_pow(e_generators(), s % R)


def chain_group(lo, hi, inf=None):
    """pairs lo .. hi - 1 of the chain, `inf` = {index within the group: shape}; -> (pairs, expectation by the closed form)"""
    A, B, a, b = chain()
    inf = inf or {}
    pairs = [infinity(inf[i - lo], A[i], B[i]) if i - lo in inf else (A[i], B[i]) for i in range(lo, hi)]
    return pairs, closed_form(sum(a[i] * b[i] for i in range(lo, hi) if i - lo not in inf))


@functools.lru_cache(None)
def size_cases():
    cases = []
    for n in SIZES:
        pairs, want = chain_group(0, n)
        cases.append(Case("size_%d" % n, [pairs], [want]))
    for n in SIZES:
        where = sorted({0, 255, 256, n - 1} & set(range(n)))
        pairs, want = chain_group(0, n, {i: INF_SHAPES[k % 3] for k, i in enumerate(where)})
        cases.append(Case("size_%d_with_inf" % n, [pairs], [want]))
    for n in (257, 513):
        pairs, want = chain_group(0, n, {i: INF_SHAPES[i % 3] for i in range(n - 1)})
        cases.append(Case("lone_pair_of_%d" % n, [pairs], [want]))
    for count in (3, 5):
        groups = [chain_group(257 * k, 257 * (k + 1)) for k in range(count)]
        cases.append(Case("count%d_n257" % count, [g for g, _ in groups], [w for _, w in groups]))
        assert len({tuple(w) for _, w in groups}) == count
    return cases


def all_cases():
    return small_cases() + size_cases()


def all_cases_recorded():
    return small_cases_recorded() + size_cases()


def plain_size_cases():
    return [c for c in size_cases() if c.name in {"size_%d" % n for n in SIZES}]


# ---------------- the native chain: fixtures, crafted and tampered proofs ----------------
def _g1_of(w):
    return (bn.u32_to_fq(w[:8]), bn.u32_to_fq(w[8:16]))


def _g2_of(w):
    return ((bn.u32_to_fq(w[:8]), bn.u32_to_fq(w[8:16])), (bn.u32_to_fq(w[16:24]), bn.u32_to_fq(w[24:32])))


def f12_of(w):
    return [bn.u32_to_fq(w[8 * i: 8 * i + 8]) for i in range(12)]


@functools.lru_cache(None)
def fixture(n):
    """(A words [n, 16], B words [n, 32], honest proof words [2 log2 n + 1, 96] in proof order) of tests/golden/sipp_n<n>_ios.npz: the
    messages are the statement's Z and the x fields of the Fq12 obligations (Z_L, Z_R round by round); the proof is their reverse"""
    d = np.load(os.path.join(GOLDEN, "sipp_n%d_ios.npz" % n))
    st = d["statement"]
    A, B = st[: 16 * n].reshape(n, 16), st[16 * n: 48 * n].reshape(n, 32)
    sent = [st[48 * n: 48 * n + 96]] + [rec[:96] for rec in d["fq12"]]
    return A, B, np.array(sent[::-1], dtype=np.uint32)


def points_of(A, B):
    return [_g1_of(a) for a in A], [_g2_of(b) for b in B]


@functools.lru_cache(None)
def provable_elements():
    """[(name, element)]: the non-zero Fq12 edge elements the catalogue of the exponentiation AIRs proves as a base"""
    proved = {tuple(r.x) for r in E.records(2)}
    return [(name, v) for name, v in E.F12_ELEMENTS if tuple(v) in proved and any(v)]


ZERO = E.F12_ELEMENTS[0][1]
assert not any(ZERO)


def proof_words(proof):
    return np.array([bn.f12_to_u32(m) for m in proof], dtype=np.uint32)


@functools.lru_cache(None)
def crafted_proofs():
    """[(name, n, proof)]: edge elements as the messages Z, Z_L, Z_R, ... (sending order; `proof` is reversed as the prover's) behind
    the honest A, B of the n = 4 fixture (its first two pairs for n = 2): three proofs at n = 2, two at n = 4, every element used"""
    els = provable_elements()
    assert len(els) == 9
    out = []
    for n, picks in ((2, (0, 1, 2)), (2, (3, 4, 5)), (2, (6, 7, 8)), (4, (0, 1, 2, 3, 4)), (4, (8, 7, 6, 5, 4))):
        out.append(("n%d_%s" % (n, "_".join(els[i][0] for i in picks[:3])), n, tuple(tuple(els[i][1]) for i in picks[::-1])))
    return out


def zero_message_proof():
    """(n, proof): Z_L = 0 between Z = 1 and Z_R = w^6, n = 2"""
    els = dict(provable_elements())
    return 2, (tuple(els["w6"]), tuple(ZERO), tuple(els["one"]))


def crafted_points(n):
    A, B, _ = fixture(4)
    return A[:n], B[:n]


@functools.lru_cache(None)
def reading(n, A_bytes, B_bytes, proof):
    A = np.frombuffer(A_bytes, dtype=np.uint32).reshape(n, 16)
    B = np.frombuffer(B_bytes, dtype=np.uint32).reshape(n, 32)
    ok, st, obl = sn.sipp_verify_native(*points_of(A, B), [list(m) for m in proof])
    return ok, np.array(sn.statement_to_u32(st), dtype=np.uint32), sn.io_records(obl)


def python_reading(A, B, proof):
    """oracle/py/sipp_native.py on word arrays (proof: words [m, 96] or tuples of coefficients) -> (accepted, statement words,
    (g1, g2, fq12) record arrays); cached within a process: several tests of one file ask for the same reading"""
    A, B = np.ascontiguousarray(A, dtype=np.uint32), np.ascontiguousarray(B, dtype=np.uint32)
    if isinstance(proof, np.ndarray):
        proof = tuple(tuple(f12_of([int(x) for x in m])) for m in proof)
    return reading(A.shape[0], A.tobytes(), B.tobytes(), proof)


def flip_top_limb(c11_top):
    """another value of the top 32-bit limb of a coefficient that keeps the coefficient below p: clear the limb's highest set bit (set
    bit 0 of an all-zero limb: 2^224 < p)"""
    return c11_top ^ (1 << (c11_top.bit_length() - 1)) if c11_top else 1


@functools.lru_cache(None)
def tampered_proofs(n=8):
    """[(name, message index, proof words)]: the honest proof of the fixture with ONE bit changed -- the lowest bit of the first
    coefficient, and a bit of the top limb of the last coefficient, of each of its 2 log2 n + 1 messages; every coefficient stays < p"""
    _, _, honest = fixture(n)
    out = []
    for m in range(honest.shape[0]):
        low, top = honest.copy(), honest.copy()
        low[m, 0] ^= 1
        top[m, 95] = flip_top_limb(int(top[m, 95]))
        for kind, pf in (("low", low), ("top", top)):
            assert all(c < P for c in f12_of([int(x) for x in pf[m]])) and (pf != honest).sum() == 1
            out.append(("%s_msg%d" % (kind, m), m, pf))
    return out


READ_TAMPERED = ("low_msg6", "top_msg0")       # (the changed Z itself; the last round's Z_R) -- the two held against the Python reading


if __name__ == "__main__":
    np.savez_compressed(SMALL_RECORDED, **{c.name: case_words(c)[3] for c in small_cases()})
    print("wrote %s (%d calls)" % (SMALL_RECORDED, len(small_cases())))
