// sipp_amd/csrc/host_keccak.hpp -- Keccak-256 truncated to 25 bytes as a Merkle hasher (plonky2 hash/keccak.rs KeccakHash<25>, as
// recalled), header-only: the host verifier (verify.cpp), the C ABI's test surface (api.hip) and the device kernels (keccak.hip)
// read the ONE permutation and the ONE packing below; a plain C++ compiler sees no HIP in it.
//
//   keccak256      original Keccak: rate 136 bytes, padding 0x01 .. 0x80 (not SHA-3's 0x06)
//   hash_no_pad    every element as its CANONICAL u64, 8 bytes little endian, concatenated; keccak256, first 25 bytes
//   hash_or_noop   at most 3 elements (24 bytes <= 25): the element bytes in a zeroed 25-byte array, nothing hashed; else hash_no_pad
//   two_to_one     keccak256 of the 50 bytes l || r (one block), first 25 bytes
//   a digest is FOUR WORDS: bytes 0..6, 7..13, 14..20, 21..24 little endian (BytesHash::to_vec): words 0 - 2 below 2^56, word 3
//   below 2^32, each a canonical field element.  The no-op form is therefore not a copy of the elements: 24 bytes re-cut by sevens.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SIPP_KECCAK_HD __host__ __device__ inline
#else
#define SIPP_KECCAK_HD inline
#endif

// loop hints for the device build (clang); another host compiler does not know the pragma
#if defined(__clang__)
#define SIPP_KECCAK_UNROLL _Pragma("unroll")
#define SIPP_KECCAK_ROLLED _Pragma("unroll 1")
#else
#define SIPP_KECCAK_UNROLL
#define SIPP_KECCAK_ROLLED
#endif

namespace keccak {

constexpr uint64_t GL_P = 0xffffffff00000001ULL;
constexpr int RATE_WORDS = 17;   // 136 bytes

SIPP_KECCAK_HD uint64_t rotl(uint64_t x, int n) { return n == 0 ? x : (x << n) | (x >> (64 - n)); }
SIPP_KECCAK_HD uint64_t canon(uint64_t x) { return x >= GL_P ? x - GL_P : x; }

// Keccak-f[1600] on lanes a[x + 5 y]; the round loop stays rolled (24 x about 330 instructions on the device)
SIPP_KECCAK_HD void f1600(uint64_t (&a)[25]) {
    static constexpr uint64_t RC[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
                                 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
                                 0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
                                 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
                                 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    static constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
SIPP_KECCAK_ROLLED
    for (int r = 0; r < 24; r++) {
        uint64_t c[5], b[25];
SIPP_KECCAK_UNROLL
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
SIPP_KECCAK_UNROLL
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1);
SIPP_KECCAK_UNROLL
            for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
        }
SIPP_KECCAK_UNROLL
        for (int x = 0; x < 5; x++)
SIPP_KECCAK_UNROLL
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], ROT[x + 5 * y]);
SIPP_KECCAK_UNROLL
        for (int y = 0; y < 5; y++)
SIPP_KECCAK_UNROLL
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= RC[r];
    }
}

// the first 25 bytes of the state as the four digest words
SIPP_KECCAK_HD void pack25(uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3, uint64_t out[4]) {
    out[0] = s0 & 0x00ffffffffffffffULL;
    out[1] = (s0 >> 56) | ((s1 & 0x0000ffffffffffffULL) << 8);
    out[2] = (s1 >> 48) | ((s2 & 0x000000ffffffffffULL) << 16);
    out[3] = (s2 >> 40) | ((s3 & 0xffULL) << 24);
}

// four digest words back to their 25 bytes: three full lanes and byte 24 (bits of a word above its range are dropped: the verifier
// refuses such a word before it gets here)
SIPP_KECCAK_HD void unpack25(const uint64_t w[4], uint64_t l[4]) {
    l[0] = (w[0] & 0x00ffffffffffffffULL) | (w[1] << 56);
    l[1] = ((w[1] >> 8) & 0x0000ffffffffffffULL) | (w[2] << 48);
    l[2] = ((w[2] >> 16) & 0x000000ffffffffffULL) | (w[3] << 40);
    l[3] = (w[3] >> 24) & 0xffULL;
}

// a digest word inside its range (words 0 - 2 below 2^56, word 3 below 2^32)?
SIPP_KECCAK_HD bool word_in_range(uint64_t w, int k) { return k < 3 ? (w >> 56) == 0 : (w >> 32) == 0; }

// hash_or_noop of n elements delivered by get(i) (any u64 congruent to the element; reduced here), one call site of the permutation
template <class Get>
SIPP_KECCAK_HD void hash_or_noop_with(uint32_t n, Get get, uint64_t out[4]) {
    if (n <= 3) {
        const uint64_t e0 = n > 0 ? canon(get(0u)) : 0, e1 = n > 1 ? canon(get(1u)) : 0, e2 = n > 2 ? canon(get(2u)) : 0;
        pack25(e0, e1, e2, 0, out);
        return;
    }
    uint64_t s[25];
SIPP_KECCAK_UNROLL
    for (int i = 0; i < 25; i++) s[i] = 0;
SIPP_KECCAK_ROLLED
    for (uint32_t c = 0;; c += RATE_WORDS) {
        const uint32_t m = n - c;   // elements left, 0 when the padding alone fills a last block
SIPP_KECCAK_UNROLL
        for (int i = 0; i < RATE_WORDS; i++)
            if ((uint32_t)i < m) s[i] ^= canon(get(c + (uint32_t)i));
        const bool last = m < (uint32_t)RATE_WORDS;
        if (last) {
SIPP_KECCAK_UNROLL
            for (int i = 0; i < RATE_WORDS; i++)
                if ((uint32_t)i == m) s[i] ^= 0x01ULL;
            s[RATE_WORDS - 1] ^= 0x8000000000000000ULL;
        }
        f1600(s);
        if (last) break;
    }
    pack25(s[0], s[1], s[2], s[3], out);
}

SIPP_KECCAK_HD void hash_or_noop(const uint64_t* e, size_t n, uint64_t out[4]) {
    hash_or_noop_with((uint32_t)n, [e](uint32_t i) { return e[i]; }, out);
}

// keccak256(l || r) of two digests (50 bytes, one block: the padding starts at byte 50), first 25 bytes
SIPP_KECCAK_HD void two_to_one(const uint64_t l[4], const uint64_t r[4], uint64_t out[4]) {
    uint64_t a[4], b[4], s[25];
    unpack25(l, a);
    unpack25(r, b);
    s[0] = a[0];
    s[1] = a[1];
    s[2] = a[2];
    s[3] = a[3] | (b[0] << 8);
    s[4] = (b[0] >> 56) | (b[1] << 8);
    s[5] = (b[1] >> 56) | (b[2] << 8);
    s[6] = (b[2] >> 56) | (b[3] << 8) | (0x01ULL << 16);
SIPP_KECCAK_UNROLL
    for (int i = 7; i < 25; i++) s[i] = 0;
    s[RATE_WORDS - 1] = 0x8000000000000000ULL;
    f1600(s);
    pack25(s[0], s[1], s[2], s[3], out);
}

// keccak256 of a byte string (host side: known answers, the test surface); out = 32 bytes
inline void keccak256(const uint8_t* in, size_t len, uint8_t out[32]) {
    uint64_t s[25];
    for (int i = 0; i < 25; i++) s[i] = 0;
    size_t at = 0;
    for (;;) {
        const size_t m = len - at < 136 ? len - at : 136;
        for (size_t i = 0; i < m; i++) s[i >> 3] ^= (uint64_t)in[at + i] << (8 * (i & 7));
        at += m;
        const bool last = m < 136;
        if (last) {
            s[m >> 3] ^= (uint64_t)0x01 << (8 * (m & 7));
            s[16] ^= 0x8000000000000000ULL;
        }
        f1600(s);
        if (last) break;
    }
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(s[i >> 3] >> (8 * (i & 7)));
}

}  // namespace keccak
