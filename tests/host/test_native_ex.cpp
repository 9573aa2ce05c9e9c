// tests/host/test_native_ex.cpp -- sipp::Prover::sipp_prove_native_ex (include/sipp_host.hpp) against the two calls it replaces.
// usage: test_native_ex points.bin     (u32 words: n, then A [n][16], then B [n][32]); compiled and run by tests/test_gpu_native_ex.py
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sipp_host.hpp"

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    CHECK(f);
    uint32_t n = 0;
    CHECK(fread(&n, 4, 1, f) == 1 && n >= 1 && n <= 4096);
    std::vector<sipp::G1Affine> A(n);
    std::vector<sipp::G2Affine> B(n);
    static_assert(sizeof(sipp::G1Affine) == 64 && sizeof(sipp::G2Affine) == 128 && sizeof(sipp::Fq12) == 384, "limb layouts");
    CHECK(fread(A.data(), sizeof(sipp::G1Affine), n, f) == n && fread(B.data(), sizeof(sipp::G2Affine), n, f) == n);
    fclose(f);
    size_t lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    try {
        sipp::Prover prover(0, n - 1, n - 1, 2 * lg);
        const std::vector<sipp::Fq12> proof = prover.sipp_prove_native(A, B);
        const auto v = prover.sipp_verify_native(A, B, proof);
        const auto r = prover.sipp_prove_native_ex(A, B);
        const auto& w = r.verification;
        CHECK(same(r.proof, proof));
        CHECK(w.g1_obligations.size() == n - 1 && w.g2_obligations.size() == n - 1 && w.fq12_obligations.size() == 2 * lg);
        CHECK(same(w.g1_obligations, v.g1_obligations) && same(w.g2_obligations, v.g2_obligations) &&
              same(w.fq12_obligations, v.fq12_obligations));
        CHECK(same(w.statement.A, A) && same(w.statement.B, B));
        CHECK(std::memcmp(&w.statement.Z, &v.statement.Z, sizeof(sipp::Fq12)) == 0);
        CHECK(std::memcmp(&w.statement.final_A, &v.statement.final_A, sizeof(sipp::G1Affine)) == 0);
        CHECK(std::memcmp(&w.statement.final_B, &v.statement.final_B, sizeof(sipp::G2Affine)) == 0);
        CHECK(std::memcmp(&w.statement.final_Z, &v.statement.final_Z, sizeof(sipp::Fq12)) == 0);
        // sizes that are no power of two are refused by the wrapper itself
        try {
            std::vector<sipp::G1Affine> A3(A.begin(), A.begin() + (n > 3 ? 3 : 0));
            std::vector<sipp::G2Affine> B3(B.begin(), B.begin() + (n > 3 ? 3 : 0));
            (void)prover.sipp_prove_native_ex(A3, B3);
            CHECK(!"a size that is no power of two was taken");
        } catch (const sipp::Error& e) {
            CHECK(e.status() == SIPP_E_BADARG);
        }
    } catch (const sipp::Error& e) {
        fprintf(stderr, "sipp::Error %d: %s\n", e.status(), e.what());
        return 1;
    }
    printf("native_ex ok: %u pairs\n", n);
    return 0;
}
