"""A Python reading of SIPP_GEN_POSEIDON_MDS (kind 16, include/sipp_hip.h) in exact integers: twelve extension elements, element c limb l
at in + 2 c + l, and out[2 r + l] = sum_c M[r][c] in[2 c + l] mod p, M the permutation's MDS matrix written out here (the circulant
first row plus 8 on the diagonal's first entry), the inputs taken as field values whatever word they hold.  It shares nothing with
sipp_amd/merkle.py.  Importing this module registers the reading in tests._witness_reading.READINGS.

  mds_row         one row's wires as a list of ints, in place
  half_sums       what the device's exact half-product sum passes through for output r of one limb: (al, ah, lo wrapped, ah >> 32)"""
from tests import _witness_reading as rd

P = 0xFFFFFFFF00000001
GEN_POSEIDON_MDS = 16
CIRC = (17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20)
M = [[CIRC[(c - r) % 12] + (8 if r == c == 0 else 0) for c in range(12)] for r in range(12)]


def mds_row(w, in_, out):
    ins = [[w[in_ + 2 * c + l] % P for c in range(12)] for l in range(2)]
    for r in range(12):
        for l in range(2):
            w[out + 2 * r + l] = sum(M[r][c] * ins[l][c] for c in range(12)) % P


def half_sums(words, r):
    """the twelve 64-bit words of one limb -> (al, ah, whether al + 2^32 ah wraps 2^64, ah >> 32) for output r"""
    al = sum((v & 0xFFFFFFFF) * M[r][c] for c, v in enumerate(words))
    ah = sum((v >> 32) * M[r][c] for c, v in enumerate(words))
    assert al < 1 << 64 and ah < 1 << 64
    lo = (al + (ah << 32)) % (1 << 64)
    return al, ah, lo < al, ah >> 32


rd.READINGS[GEN_POSEIDON_MDS] = rd._row_by_row(lambda w, p, c: mds_row(w, p[0], p[1]))
