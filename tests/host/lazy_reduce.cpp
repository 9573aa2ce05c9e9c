// tests/host/lazy_reduce.cpp -- gl::reduce6 (sipp_amd/csrc/gl.hpp: the two-chain reduction behind gl::Acc6::reduce, the SAME code the
// device compiles) against unsigned __int128 arithmetic mod p.  CPU only; tests/test_host_lazy_reduce.py builds and runs it, plain and
// under AddressSanitizer + UBSan.
//   value = a0 + a1 2^22 + a2 2^44 + 2^32 (a3 + a4 2^22 + a5 2^44)   ->   any u64 congruent to it
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "gl.hpp"

typedef unsigned __int128 u128;

static uint64_t mod_p(u128 x) { return (uint64_t)(x % (u128)gl::P); }

// the value mod p, term by term (every term reduced first: nothing here can overflow 128 bits)
static uint64_t want(const uint64_t (&a)[6]) {
    static const unsigned shift[6] = {0, 22, 44, 32, 54, 76};
    u128 s = 0;
    for (int i = 0; i < 6; i++) s += (u128)mod_p(a[i]) * mod_p((u128)1 << shift[i]) % (u128)gl::P;
    return mod_p(s);
}

static long checked = 0;
static int check(const uint64_t (&a)[6], const char* what) {
    const uint64_t got = gl::reduce6(a), w = want(a);
    checked++;
    if (mod_p(got) == w) return 0;
    std::printf("MISMATCH (%s): a = %016llx %016llx %016llx %016llx %016llx %016llx  got %016llx (mod p %016llx)  want %016llx\n", what,
                (unsigned long long)a[0], (unsigned long long)a[1], (unsigned long long)a[2], (unsigned long long)a[3], (unsigned long long)a[4],
                (unsigned long long)a[5], (unsigned long long)got, (unsigned long long)mod_p(got), (unsigned long long)w);
    return 1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t splitmix() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 100000;
    int bad = 0;
    const uint64_t M60 = ((uint64_t)1 << 60) - 1, M64 = ~(uint64_t)0;
    {
        uint64_t a[6] = {0, 0, 0, 0, 0, 0};
        bad += check(a, "all zero");
    }
    // every accumulator at the hash kernels' bound, and at the words' own (Acc6 filled with 1024 worst-case products)
    for (uint64_t top : {M60, M64}) {
        uint64_t a[6] = {top, top, top, top, top, top};
        bad += check(a, "all at the maximum");
        for (int i = 0; i < 6; i++) {
            uint64_t b[6] = {0, 0, 0, 0, 0, 0};
            b[i] = top;
            bad += check(b, "one accumulator at the maximum");
            // everything BUT one at the maximum: the chains' extremes (L lowest with a0 = a1 = 0, highest with a2 .. a5 = 0)
            uint64_t c[6] = {top, top, top, top, top, top};
            c[i] = 0;
            bad += check(c, "all but one at the maximum");
        }
    }
    // each 32-bit half alone at its maximum: the low halves 2^32 - 1, the high halves 2^28 - 1 (a < 2^60) and 2^32 - 1 (any u64)
    for (int i = 0; i < 6; i++) {
        for (uint64_t v : {(uint64_t)0xFFFFFFFFull, (uint64_t)0x0FFFFFFFull << 32, (uint64_t)0xFFFFFFFFull << 32}) {
            uint64_t b[6] = {0, 0, 0, 0, 0, 0};
            b[i] = v;
            bad += check(b, "one half at its maximum");
        }
    }
    // what keeps L positive: only the subtracted halves (h2, h3, h4, l5, h5) set, and only the added ones
    {
        uint64_t a[6] = {0, 0, M64 << 32, M64 << 32, M64 << 32, M64};
        bad += check(a, "subtracted halves only");
        uint64_t b[6] = {M64, M64, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0};
        bad += check(b, "added halves only");
    }
    for (long t = 0; t < n_random; t++) {
        uint64_t a[6];
        const uint64_t mask = (t & 1) ? M64 : M60;              // half below 2^60, half any u64
        for (int i = 0; i < 6; i++) a[i] = splitmix() & mask;
        bad += check(a, "random");
        if (bad > 20) break;
    }
    std::printf("lazy_reduce: %ld sextuples, %d mismatches\n", checked, bad);
    if (!bad) std::printf("lazy_reduce ok\n");
    return bad ? 1 : 0;
}
