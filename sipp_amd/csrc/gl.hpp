// sipp_amd/csrc/gl.hpp -- Goldilocks field (p = 2^64 - 2^32 + 1) and its quadratic extension
// F_p[X]/(X^2 - 7) for gfx950 device code and the host-side driver.
//
// All values that cross a kernel boundary are canonical (< p).  64-bit integer modular
// arithmetic on a 32-bit VALU: a mulmod is four 32x32->64 multiply-adds plus a
// shift/add reduction (2^64 = 2^32 - 1, 2^96 = -1 mod p) -- no MFMA anywhere.
//
// Replaces (on the GPU side) plonky2's GoldilocksField @ InternetMaximalism/plonky2 541e127
// (reference Cargo.toml:21; used as `F` at reference src/prover_native.rs:7,12).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GL_HD __host__ __device__ __forceinline__
#else
#define GL_HD inline
#endif

namespace gl {

constexpr uint64_t P = 0xFFFFFFFF00000001ULL;
constexpr uint64_t EPS = 0xFFFFFFFFULL;  // 2^64 mod p
constexpr uint64_t GEN = 7;              // multiplicative generator == coset shift
constexpr uint64_t TWO_ADIC_ROOT = 1753635133440165772ULL;  // order 2^32
constexpr uint64_t EXT_W = 7;            // X^2 = 7

GL_HD uint64_t canon(uint64_t a) { return a >= P ? a - P : a; }

GL_HD uint64_t add(uint64_t a, uint64_t b) {
    uint64_t s = a + b;
    uint64_t t = s - P;  // == s + EPS mod 2^64
    return (s < a || s >= P) ? t : s;
}

GL_HD uint64_t sub(uint64_t a, uint64_t b) {
    uint64_t d = a - b;
    return a < b ? d + P : d;
}

GL_HD uint64_t neg(uint64_t a) { return a ? P - a : 0; }

GL_HD uint64_t dbl(uint64_t a) { return add(a, a); }

// (hi, lo) -> [0, 2^64), congruent mod p but NOT necessarily canonical.  hi:lo is any 128-bit value.
// x = lo + 2^64 hl + 2^96 hh  ==  lo - (hh + hl) + (hl << 32)      (2^64 = 2^32 - 1, 2^96 = -1)
// The borrow of the subtraction and the carry of the addition are netted into ONE correction of +-(2^32 - 1).
// (The correction as corr * EPS costs a fifth v_mad_u64_u32; two selects on the carry / borrow masks + one 64-bit addition
// have one instruction fewer and are SLOWER: 1.63-1.71 against 1.73-1.75 G leaf permutations/s, 65.5 against 62.3 ms per
// n = 128 instance -- round 2, same box, alternating.)
GL_HD uint64_t reduce128_nc(uint64_t hi, uint64_t lo) {
    const uint32_t hl = (uint32_t)hi, hh = (uint32_t)(hi >> 32);
    const uint32_t l0 = (uint32_t)lo, l1 = (uint32_t)(lo >> 32);
    uint32_t s0 = hh + hl;
    const uint32_t s1 = s0 < hh;
    const uint32_t a0 = l0 - s0;
    const uint32_t bw0 = l0 < s0;
    const uint32_t a1a = l1 - s1;
    const uint32_t a1 = a1a - bw0;
    const bool b1 = (l1 < s1) | (a1a < bw0);
    const uint32_t b1h = a1 + hl;
    const bool c1 = b1h < a1;
    const uint64_t b = ((uint64_t)b1h << 32) | a0;
    const int32_t corr = (int32_t)c1 - (int32_t)b1;  // -1, 0, +1
    return b + (uint64_t)((int64_t)corr * (int64_t)EPS);
}

GL_HD uint64_t reduce128(uint64_t hi, uint64_t lo) { return canon(reduce128_nc(hi, lo)); }

// value = lo + 2^64 * hi32 with hi32 < 2^32 (a "96-bit" accumulator) -> [0, 2^64), not canonical
GL_HD uint64_t reduce96_nc(uint32_t hi32, uint64_t lo) {
    uint64_t t1 = ((uint64_t)hi32 << 32) - hi32;
    uint64_t r = lo + t1;
    if (r < lo) r += EPS;
    return r;
}
GL_HD uint64_t reduce96(uint32_t hi32, uint64_t lo) { return canon(reduce96_nc(hi32, lo)); }

// 64 x 64 -> 128: four 32 x 32 + 64 multiply-adds (v_mad_u64_u32), no separate low product
GL_HD void mul_wide(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    const uint64_t t0 = (uint64_t)a0 * b0;
    const uint64_t t1 = (uint64_t)a0 * b1 + (t0 >> 32);
    const uint64_t t2 = (uint64_t)a1 * b0 + (uint32_t)t1;
    hi = (uint64_t)a1 * b1 + (t1 >> 32) + (t2 >> 32);
    lo = (t2 << 32) | (uint32_t)t0;
#else
    unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// product in [0, 2^64), not canonical; inputs may be any u64
GL_HD uint64_t mul_nc(uint64_t a, uint64_t b) {
    uint64_t hi, lo;
    mul_wide(a, b, hi, lo);
    return reduce128_nc(hi, lo);
}

GL_HD uint64_t mul(uint64_t a, uint64_t b) { return canon(mul_nc(a, b)); }

GL_HD uint64_t sqr(uint64_t a) { return mul(a, a); }

// a * b + c
GL_HD uint64_t mad_nc(uint64_t a, uint64_t b, uint64_t c) {
    uint64_t hi, lo;
    mul_wide(a, b, hi, lo);
    lo += c;
    hi += (lo < c);
    return reduce128_nc(hi, lo);
}
GL_HD uint64_t mad(uint64_t a, uint64_t b, uint64_t c) { return canon(mad_nc(a, b, c)); }
// a (any u64) + c (canonical) -> [0, 2^64)
GL_HD uint64_t add_nc(uint64_t a, uint64_t c) {
    uint64_t s = a + c;
    return s < a ? s + EPS : s;
}

GL_HD uint64_t pow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    while (e) {
        if (e & 1) r = mul(r, a);
        a = sqr(a);
        e >>= 1;
    }
    return r;
}

// a^(p - 2) with the addition chain for p - 2 = 2^64 - 2^32 - 1 = (31 ones) 0 (32 ones): 63 squarings + 9 products
// instead of the 126 of square-and-multiply.  inv(0) = 0.
GL_HD uint64_t sqr_n(uint64_t a, int n) {
    for (int i = 0; i < n; i++) a = mul_nc(a, a);
    return a;
}
GL_HD uint64_t inv(uint64_t a) {
    const uint64_t t2 = mul_nc(mul_nc(a, a), a);            // 2 ones
    const uint64_t t3 = mul_nc(mul_nc(t2, t2), a);          // 3 ones
    const uint64_t t6 = mul_nc(sqr_n(t3, 3), t3);
    const uint64_t t12 = mul_nc(sqr_n(t6, 6), t6);
    const uint64_t t24 = mul_nc(sqr_n(t12, 12), t12);
    const uint64_t t30 = mul_nc(sqr_n(t24, 6), t6);
    const uint64_t t31 = mul_nc(mul_nc(t30, t30), a);       // 31 ones
    const uint64_t t63 = mul_nc(sqr_n(t31, 32), t31);       // (31 ones)(0)(31 ones)
    return mul(mul_nc(t63, t63), a);                        // (31 ones)(0)(32 ones)
}

GL_HD uint64_t root_of_unity(unsigned k) {
    uint64_t r = TWO_ADIC_ROOT;
    for (unsigned i = k; i < 32; i++) r = sqr(r);
    return r;
}

// signed integer -> field; the magnitude of a negative v is taken in uint64_t (-v overflows for INT64_MIN)
GL_HD uint64_t from_i64(int64_t v) { return v >= 0 ? (uint64_t)v : P - (0 - (uint64_t)v); }

// ---- the reduction of the lazy dot products (Acc6 below) as two 64-bit chains ----
// value = a[0] + a[1] 2^22 + a[2] 2^44 + 2^32 (a[3] + a[4] 2^22 + a[5] 2^44) with a[i] = l_i + 2^32 h_i.  The twelve halves go into
// two chains L (weight 1) and H (weight 2^32) with weights 1, 2^12 and 2^22 only (2^64 = 2^32 - 1, 2^96 = -1 mod p):
//   N' = 2^12 h2 + h3 + 2^22 h4 + 2^12 l5          (enters H with +, L with -: each word of weight 2^64 is worth 2^32 - 1)
//   L  = L0 + l0 + 2^22 l1 - N' - 2^12 h5
//   H  = H0 + h0 + 2^22 h1 + 2^12 l2 + l3 + 2^22 l4 + N'
// L0 = 2^56 - 2^32 + 1 and H0 = 2^32 - 2^24 (L0 + 2^32 H0 = p) keep L positive.  Input bound: NONE beyond the words themselves -- the
// a[i] may be any u64 (Acc6's 1024 products; the hash kernels stay below 2^60): what L loses is below 2^54 + 2^46, L < 2^57, H < 2^56.
// The fold: L + 2^32 H = L + (H >> 32)(2^32 - 1) + 2^32 lo(H) is one multiply-add (< 2^58) and one addition into the high word, whose
// carry (2^64) is repaid by + (2^32 - 1); that cannot wrap, the high word after a carry is below 2^26.
// Thirteen multiply-adds (the fold's among them), a 64-bit addition and subtraction, four instructions for the fold's carry and the
// moves of L0 and H0: 24 instructions (scripts/count_valu.py scripts/ubench/acc6_reduce.hip).
// On the device 1, 2^12 and 2^22 are opaque wave-uniform values: as literals the compiler spells the multiply-adds as 64-bit shifts and
// split additions with zero-extension moves.
// -> [0, 2^64), congruent to the value, not canonical.
#if defined(__HIP_DEVICE_COMPILE__)
#define GL_CHAIN_STEP(x) asm("" : "+v"(x))    /* one multiply-add per term: keeps the compiler from regrouping the chains */
#else
#define GL_CHAIN_STEP(x) (void)0
#endif
GL_HD uint64_t reduce6(const uint64_t (&a)[6]) {
    uint32_t z = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(z));
#endif
    const uint32_t p1 = 1u + z, p12 = (1u << 12) + z, p22 = (1u << 22) + z;
    const uint32_t l0 = (uint32_t)a[0], l1 = (uint32_t)a[1], l2 = (uint32_t)a[2], l3 = (uint32_t)a[3], l4 = (uint32_t)a[4], l5 = (uint32_t)a[5];
    const uint32_t h0 = (uint32_t)(a[0] >> 32), h1 = (uint32_t)(a[1] >> 32), h2 = (uint32_t)(a[2] >> 32);
    const uint32_t h3 = (uint32_t)(a[3] >> 32), h4 = (uint32_t)(a[4] >> 32), h5 = (uint32_t)(a[5] >> 32);
    uint64_t n = (uint64_t)h3 * p1;
    GL_CHAIN_STEP(n);
    n = (uint64_t)h2 * p12 + n;
    GL_CHAIN_STEP(n);
    n = (uint64_t)h4 * p22 + n;
    GL_CHAIN_STEP(n);
    n = (uint64_t)l5 * p12 + n;                                     // N' < 2^55
    GL_CHAIN_STEP(n);
    uint64_t H = (uint64_t)h0 * p1 + 0xFF000000ULL;                 // H0
    GL_CHAIN_STEP(H);
    H = (uint64_t)l3 * p1 + H;
    GL_CHAIN_STEP(H);
    H = (uint64_t)l2 * p12 + H;
    GL_CHAIN_STEP(H);
    H = (uint64_t)h1 * p22 + H;
    GL_CHAIN_STEP(H);
    H = (uint64_t)l4 * p22 + H;
    GL_CHAIN_STEP(H);
    H += n;
    uint64_t L = (uint64_t)l0 * p1 + 0x00FFFFFF00000001ULL;         // L0
    GL_CHAIN_STEP(L);
    L = (uint64_t)l1 * p22 + L;
    GL_CHAIN_STEP(L);
    uint64_t m = (uint64_t)h5 * p12 + n;
    GL_CHAIN_STEP(m);
    L -= m;
    const uint64_t t = (uint64_t)(uint32_t)(H >> 32) * (uint32_t)EPS + L;
    const uint32_t th = (uint32_t)(t >> 32), mid = th + (uint32_t)H;
    const uint64_t r = ((uint64_t)mid << 32) | (uint32_t)t;
    return mid < th ? r + EPS : r;
}
#undef GL_CHAIN_STEP

#if defined(__HIPCC__)
#define GL_D __device__ __forceinline__
// ---- lazy dot products on the 32-bit VALU ----
// sum of (64-bit value x) x (64-bit value c) products with c cut into limbs c0 + c1 2^22 + c2 2^44 (22 + 22 + 20 bits):
// value = a[0] + a[1] 2^22 + a[2] 2^44 + 2^32 (a[3] + a[4] 2^22 + a[5] 2^44).  Each product is < 2^54, so a[] holds
// 1024 of them.
struct Acc6 {
    uint64_t a[6];
    GL_D void zero() {
#pragma unroll
        for (int j = 0; j < 6; j++) a[j] = 0;
    }
    GL_D void set(uint32_t lo, uint32_t hi) {
        zero();
        a[0] = lo;
        a[3] = hi;
    }
    GL_D void mac(uint32_t xl, uint32_t xh, const uint32_t* __restrict__ c) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            a[j] += (uint64_t)xl * c[j];
            a[3 + j] += (uint64_t)xh * c[j];
        }
    }
    // -> [0, 2^64), congruent to the value, not canonical; the a[] may be any u64 (reduce6 above)
    GL_D uint64_t reduce() const { return reduce6(a); }
};

// sum of full 64 x 64 products (both factors per-lane values) in 160 bits, one reduction at the end
struct Acc160 {
    uint64_t lo = 0, hi = 0;
    uint32_t c = 0;
    GL_D void mac(uint64_t a, uint64_t b) {
        uint64_t ph, pl;
        mul_wide(a, b, ph, pl);
        lo += pl;
        ph += (lo < pl);  // ph <= 2^64 - 2, cannot wrap
        hi += ph;
        c += (hi < ph);
    }
    // 2^128 = -2^32 (mod p); result in [0, 2^64), not canonical
    GL_D uint64_t reduce() const {
        const uint64_t r = reduce128_nc(hi, lo), t = (uint64_t)c << 32;
        const uint64_t d = r - t;
        return r < t ? d - EPS : d;  // r < t < 2^37: d wrapped is >= 2^64 - 2^37 > EPS
    }
};

// c -> limbs for Acc6::mac (the host builds the tables of constant weights with it)
GL_HD void limbs3(uint32_t (&o)[3], uint64_t c) {
    o[0] = (uint32_t)c & 0x3FFFFFu;
    o[1] = (uint32_t)(c >> 22) & 0x3FFFFFu;
    o[2] = (uint32_t)(c >> 44);
}
#endif

// ---- quadratic extension ----
struct E2 {
    uint64_t c0, c1;
};

GL_HD E2 e2(uint64_t c0, uint64_t c1 = 0) { return E2{c0, c1}; }
GL_HD E2 add(E2 a, E2 b) { return E2{add(a.c0, b.c0), add(a.c1, b.c1)}; }
GL_HD E2 sub(E2 a, E2 b) { return E2{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
GL_HD E2 neg(E2 a) { return E2{neg(a.c0), neg(a.c1)}; }
GL_HD E2 mul(E2 a, E2 b) {
    uint64_t t = mul(a.c1, b.c1);
    uint64_t c0 = mad(a.c0, b.c0, mul(t, EXT_W));
    uint64_t c1 = mad(a.c0, b.c1, mul(a.c1, b.c0));
    return E2{c0, c1};
}
GL_HD E2 scale(E2 a, uint64_t s) { return E2{mul(a.c0, s), mul(a.c1, s)}; }
GL_HD E2 sqr(E2 a) { return mul(a, a); }
GL_HD bool eq(E2 a, E2 b) { return a.c0 == b.c0 && a.c1 == b.c1; }
GL_HD E2 inv(E2 a) {
    uint64_t n = sub(sqr(a.c0), mul(EXT_W, sqr(a.c1)));
    uint64_t ni = inv(n);
    return E2{mul(a.c0, ni), mul(neg(a.c1), ni)};
}
GL_HD E2 pow(E2 a, uint64_t e) {
    E2 r{1, 0};
    while (e) {
        if (e & 1) r = mul(r, a);
        a = sqr(a);
        e >>= 1;
    }
    return r;
}

GL_HD uint32_t bitrev(uint32_t x, unsigned bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return bits ? (__brev(x) >> (32 - bits)) : 0;
#else
    uint32_t r = 0;
    for (unsigned i = 0; i < bits; i++) {
        r = (r << 1) | (x & 1);
        x >>= 1;
    }
    return r;
#endif
}

}  // namespace gl
