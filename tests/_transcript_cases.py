"""The u32 and nonnative witness generators (kinds 19 - 21, include/sipp_hip.h) read in exact Python integers, the catalogue of rows that
reaches their edges, and the reference's SIPP transcript with eight fixed limbs per challenge.  Shares nothing with sipp_amd/nonnative.py
or the device code.  Importing this module registers the three readings in tests._witness_reading.READINGS.

  u32_arithmetic_row, u32_add_many_row, nonnative_row   one row's wires as a list of ints, in place
  CATALOGUE          name -> (kind, inputs): the rows every launch path is run over
  catalogue_table    the catalogue as one wire table: (wires, constants, generators, the reading's table, row names)
  transcript         the reference's transcript_native.rs over words, every challenge read as eight limbs: [(x, x^-1)] per round
  fixture            tests/golden/sipp_n<n>_ios.npz -> (statement words, round words, the recorded exponents per round)"""
import os

import numpy as np

from tests import _challenger_reading  # noqa: F401 (registers the reading of SIPP_GEN_BASE_SUM, the circuit's le_sum rows)
from tests import _witness_reading as rd

P = 0xFFFFFFFF00000001
M32 = 0xFFFFFFFF
GEN_U32_ARITHMETIC, GEN_U32_ADD_MANY, GEN_NONNATIVE = 19, 20, 21
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # the BN254 scalar prime
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583      # the BN254 base prime
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def limbs(v, n=8):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * k)) & M32 for k in range(n)]


def value(ls):
    return sum((int(x) & M32) << (32 * k) for k, x in enumerate(ls))


def u32_arithmetic_row(w, n_ops, stride, n_limbs):
    for op in range(n_ops):
        b = stride * op
        full = (w[b] & M32) * (w[b + 1] & M32) + (w[b + 2] & M32)
        lo, hi = full & M32, full >> 32
        w[b + 3], w[b + 4] = lo, hi
        w[b + 5] = pow(M32 - hi, P - 2, P)                     # 0 for hi = 2^32 - 1
        for h, half in enumerate((lo, hi)):
            for l in range(n_limbs):
                w[b + 6 + n_limbs * h + l] = (half >> (2 * l)) & 3


def u32_add_many_row(w, n_ops, stride, n_addends, n_carry_limbs):
    for op in range(n_ops):
        b = stride * op
        total = sum(w[b + k] & M32 for k in range(n_addends + 1))
        lo, carry = total & M32, total >> 32
        w[b + n_addends + 1], w[b + n_addends + 2] = lo, carry
        for l in range(16):
            w[b + n_addends + 3 + l] = (lo >> (2 * l)) & 3
        for l in range(n_carry_limbs):
            w[b + n_addends + 19 + l] = (carry >> (2 * l)) & 3


def gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def nonnative(op, x, m):
    """-> (result, quotient, slack) as integers, or None for a refused row"""
    if m == 0:
        return None
    if op == 0:
        return x % m, x // m, m - 1 - x % m
    if m % 2 == 0 or m == 1 or gcd(x % m, m) != 1:
        return None
    inv = pow(x % m, -1, m)
    assert (x * inv - 1) % m == 0
    return inv, (x * inv - 1) // m, m - 1 - inv


def nonnative_row(w, op, x0, m0, out0):
    got = nonnative(op, value(w[x0:x0 + 8]), value(w[m0:m0 + 8]))
    w[out0:out0 + 24] = [0] * 24 if got is None else limbs(got[0]) + limbs(got[1]) + limbs(got[2])


rd.READINGS[GEN_U32_ARITHMETIC] = rd._row_by_row(lambda w, p, c: u32_arithmetic_row(w, p[0], p[1], p[2]))
rd.READINGS[GEN_U32_ADD_MANY] = rd._row_by_row(lambda w, p, c: u32_add_many_row(w, p[0], p[1], p[2], p[3]))
rd.READINGS[GEN_NONNATIVE] = rd._row_by_row(lambda w, p, c: nonnative_row(w, p[0], p[1], p[2], p[3]))

# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
# the generators of the table: selector column 0, value = 1 + position.  Arithmetic: two ops of stride 38 with sixteen limbs per half;
# add-many: one op of sixteen addends and three carry limbs; reduce and inverse: x at 0, m at 8, the 24 outputs from 16.
NUM_WIRES = 135
ARITH = (GEN_U32_ARITHMETIC, 0, 1, 2, 38, 16, 0, 0)
ADD_MANY = (GEN_U32_ADD_MANY, 0, 2, 1, 38, 16, 3, 0)
REDUCE = (GEN_NONNATIVE, 0, 3, 0, 0, 8, 16, 0)
INVERSE = (GEN_NONNATIVE, 0, 4, 1, 0, 8, 16, 0)
GENS = [ARITH, ADD_MANY, REDUCE, INVERSE]
OTHER = 99                                                      # the selector value of a row no generator holds
FULL = (0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95) % (1 << 256)

CATALOGUE = {
    # (a, b, c) of op 0; op 1 takes the same operands rotated
    "arith_all_ones": ("arith", (M32, M32, M32)),               # the value p - 1: hi all ones, lo 0, inverse cell 0
    "arith_all_zero": ("arith", (0, 0, 0)),
    "arith_value_2^32-2": ("arith", (1, M32 - 1, 0)),           # the largest value whose other split (V + p) fits 64 bits
    "arith_value_2^32": ("arith", (1 << 16, 1 << 16, 0)),
    "arith_value_2^32_by_the_addend": ("arith", (1, M32, 1)),
    "arith_bits_above_32": ("arith", ((5 << 32) | 7, (1 << 63) | 11, P - 1)),
    "arith_hi_all_ones_lo_zero_again": ("arith", (M32, M32, M32)),
    # sixteen addends, then the carry-in
    "add_all_maxima": ("add", [M32] * 17),                      # 17 (2^32 - 1): carry-out 16, the largest
    "add_single_addend": ("add", [0x89ABCDEF] + [0] * 16),
    "add_zero": ("add", [0] * 17),
    "add_carry_in_only": ("add", [0] * 16 + [M32]),
    "add_bits_above_32": ("add", [(3 << 32) | 1] * 16 + [(1 << 40) | 2]),
    # (x, m)
    "reduce_r_0": ("reduce", (0, R)), "reduce_r_1": ("reduce", (1, R)), "reduce_r_r-1": ("reduce", (R - 1, R)),
    "reduce_r_r": ("reduce", (R, R)), "reduce_r_r+1": ("reduce", (R + 1, R)), "reduce_r_2r+5": ("reduce", (2 * R + 5, R)),
    "reduce_r_3r+5": ("reduce", (3 * R + 5, R)), "reduce_r_4r+9": ("reduce", (4 * R + 9, R)),
    "reduce_r_5r-1": ("reduce", (5 * R - 1, R)), "reduce_r_5r": ("reduce", (5 * R, R)),
    "reduce_r_2^256-1": ("reduce", ((1 << 256) - 1, R)),
    "reduce_r_limbs_of_0_and_ones": ("reduce", (value([0, M32, 0, M32, M32, 0, 0, M32]), R)),
    "reduce_q_full": ("reduce", (FULL, Q)), "reduce_q_q-1": ("reduce", (Q - 1, Q)), "reduce_q_2^256-1": ("reduce", ((1 << 256) - 1, Q)),
    "reduce_3_full": ("reduce", (FULL, 3)), "reduce_3_2^256-1": ("reduce", ((1 << 256) - 1, 3)), "reduce_1_full": ("reduce", (FULL, 1)),
    "reduce_m_2^256-1": ("reduce", ((1 << 256) - 2, (1 << 256) - 1)),
    "reduce_refused_m_0": ("reduce", (FULL, 0)),
    "inverse_r_1": ("inverse", (1, R)), "inverse_r_2": ("inverse", (2, R)), "inverse_r_r-1": ("inverse", (R - 1, R)),
    "inverse_r_r+1": ("inverse", (R + 1, R)), "inverse_r_full": ("inverse", (FULL, R)),
    "inverse_q_full": ("inverse", (FULL, Q)),
    "inverse_3_2": ("inverse", (2, 3)), "inverse_3_full": ("inverse", (FULL - FULL % 3 + 1, 3)),
    "inverse_m_2^256-1": ("inverse", ((1 << 256) - 2, (1 << 256) - 1)),
    "inverse_refused_m_0": ("inverse", (5, 0)), "inverse_refused_m_even": ("inverse", (5, R + 1)),
    "inverse_refused_m_1": ("inverse", (5, 1)), "inverse_refused_x_0": ("inverse", (0, R)),
    "inverse_refused_x_multiple_of_m": ("inverse", (3 * R, R)), "inverse_refused_gcd": ("inverse", (5, 15)),
}
REFUSED = sorted(k for k in CATALOGUE if "refused" in k)


def case_row(name, rng):
    """(selector value, the row's wires before generation): every cell the case does not set is a random field value"""
    kind, arg = CATALOGUE[name]
    w = [int(v) for v in rng.integers(0, P, NUM_WIRES, dtype=np.uint64)]
    if kind == "arith":
        w[0:3] = arg
        w[38:41] = arg[1:] + arg[:1]
        return 1, w
    if kind == "add":
        w[0:17] = arg
        return 2, w
    x, m = arg
    hi = int(rng.integers(0, 1 << 32)) << 32                    # operands are taken by their low 32 bits: the high halves are noise
    w[0:8] = [l | hi for l in limbs(x)]
    w[8:16] = [l | hi for l in limbs(m)]
    return 3 if kind == "reduce" else 4, w


def catalogue_table(log_n, seed=1901, repeat=True):
    """(wires, constants, GENS, want, names): row r holds case r % len(CATALOGUE) (repeat) or only the first len(CATALOGUE) rows hold
    one; every seventh row and every other row holds no generator.  want = the reading of every held row."""
    n, names = 1 << log_n, sorted(CATALOGUE)
    rng = np.random.default_rng(seed)
    w = rng.integers(0, P, (NUM_WIRES, n), dtype=np.uint64)
    k = np.full((1, n), OTHER, dtype=np.uint64)
    held = []
    for r in range(n if repeat else len(names)):
        if repeat and r % 7 == 6 and r >= len(names):
            continue
        sel, row = case_row(names[r % len(names)], rng)
        w[:, r] = np.array(row, dtype=np.uint64)
        k[0, r] = sel
        held.append(r)
    want = rd.row_local(w, k, GENS, None)
    return w, k, GENS, want, [names[r % len(names)] for r in held]


# ---- the transcript ---------------------------------------------------------------------------------------------------------------------
def transcript(hash_no_pad, statement_words, round_words):
    """reference src/transcript_native.rs over words, with the circuit's reading of a challenge: the four digest words as EIGHT u32 limbs
    (the native to_u32_digits drops a zero high half, SURVEY a14: the two agree unless a digest word is below 2^32).
    statement_words = A (16 n) || B (32 n) || Z (96); round_words = Z_L (96) || Z_R (96) per round -> ([(x, x^-1)], [digest], perms)"""
    st = [int(v) for v in statement_words]
    n = (len(st) - 96) // 48
    assert len(st) == 48 * n + 96 and n >= 2 and n & (n - 1) == 0
    rw = [int(v) for v in round_words]
    rounds = n.bit_length() - 1
    assert len(rw) == 192 * rounds
    state, perms = [0, 0, 0, 0], 0

    def append(msg):
        nonlocal state, perms
        state = [int(v) for v in hash_no_pad(state + list(msg))]
        perms += -(-(4 + len(msg)) // 8)
    for i in range(n):
        append(st[16 * i:16 * i + 16])
        append(st[16 * n + 32 * i:16 * n + 32 * i + 32])
    append(st[48 * n:])
    out, digests = [], []
    for k in range(rounds):
        append(rw[192 * k:192 * k + 96])
        append(rw[192 * k + 96:192 * k + 192])
        digest = [int(v) for v in hash_no_pad(state)]
        perms += 1
        b = sum(d << (64 * i) for i, d in enumerate(digest))
        x = b % R
        out.append((x, pow(x, R - 2, R)))
        digests.append(digest)
    return out, digests, perms


def fixture(n):
    """tests/golden/sipp_n<n>_ios.npz -> (statement words A || B || Z, round words, [(x, x^-1)] recorded per round, the npz)"""
    d = np.load(os.path.join(GOLDEN, "sipp_n%d_ios.npz" % n))
    st = [int(v) for v in d["statement"][:48 * n + 96]]
    fq = d["fq12"]
    rounds = n.bit_length() - 1
    assert fq.shape == (2 * rounds, 296)
    rw, ex = [], []
    for k in range(rounds):
        rw += [int(v) for v in fq[2 * k, :96]] + [int(v) for v in fq[2 * k + 1, :96]]
        ex.append((value(fq[2 * k, 192:200]), value(fq[2 * k + 1, 192:200])))
    return st, rw, ex, d
