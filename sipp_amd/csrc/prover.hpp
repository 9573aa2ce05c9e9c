// sipp_amd/csrc/prover.hpp -- host entry points of the prover kernels (prover.hip, poseidon.hip) and the
// host-side Fiat-Shamir challenger.
#pragma once
#include <functional>
#include <utility>

#include "commit.hpp"
#include "host_challenger.hpp"
#include "host_poseidon.hpp"
#include "poseidon_constants.h"

// quotient_rest over a thin quotient domain (2N <= 2^15 points) walks its checked columns in up to sixteen ranges of at least 32 and
// needs chunks x 6 sums per point of scratch; ONE rule for the kernel launch (prover.hip) and the arena size (stark.hip)
inline uint32_t sipp_quotient_rest_chunks(uint32_t log_n, int n_checked) {
    if (log_n + 1 > 15) return 1;
    const int c = n_checked / 32 < 16 ? n_checked / 32 : 16;
    return c > 1 ? (uint32_t)c : 1;
}
int sipp_k_z_columns(sipp_ctx* ctx, const air_spec_t* a, const uint64_t* d_trace, uint32_t log_n, const uint64_t beta[2],
                     const uint64_t gamma[2], uint64_t* d_zv);
// quotient on the coset 7 <w_2N> (the first 2N leaves of the LDEs, whose columns are lde_stride apart); d_aux [n_aux][2N],
// d_out [2][2N] in leaf order
int sipp_k_quotient(sipp_ctx* ctx, const air_spec_t* a, uint32_t log_n, const uint64_t* d_lde, const uint64_t* d_zlde,
                    size_t lde_stride, const uint64_t* d_aux, const uint64_t alpha[2], const uint64_t beta[2],
                    const uint64_t gamma[2], uint64_t* d_out);
// count (1 .. 4) tables of base[i]^k, k < n, in one launch
int sipp_k_pow_tables(sipp_ctx* ctx, const gl::E2* base, uint64_t* const* d_tab, int count, size_t n);
// (scratch of the grouped form: at most SIPP_OPENINGS_MAX_SEGS x 4 words per column -- sipp_workspace_bytes_cfg counts them)
constexpr size_t SIPP_OPENINGS_MAX_SEGS = 32;
// a gadget of more than 64 products is evaluated by up to this many lanes per quotient point (prover.hip: slices of its product list)
constexpr int SIPP_QUOTIENT_MAX_SLICES = 8;
// the columns of up to three oracles, concatenated, at the points of the tables d_t0 and d_t1 (NULL: one point; oracle 2 is opened
// at the first point only): d_out [column][4].  stark: the launch shape of a STARK's three oracles, else that of a generic range
int sipp_k_openings(sipp_ctx* ctx, const uint64_t* const d_coeffs[3], const uint32_t ncols[3], size_t n, const uint64_t* d_t0,
                    const uint64_t* d_t1, uint64_t* d_out, bool stark);
int sipp_k_fri_final(sipp_ctx* ctx, const uint64_t* const src[3], const int cnt[3], size_t n, const uint32_t* d_apow3,
                     int n1, gl::E2 shift1, const uint64_t* d_zp[2], const uint64_t* d_zip[2], uint64_t* d_final);
int sipp_k_fri_batch_quotient(sipp_ctx* ctx, const uint64_t* const* d_cols, int total, size_t n, const uint32_t* d_apow3,
                              const uint64_t* d_zp, const uint64_t* d_zip, gl::E2 shift, bool first, uint64_t* d_acc);
int sipp_k_fri_mulx(sipp_ctx* ctx, const uint64_t* d_acc, size_t n, uint64_t* d_final);
int sipp_k_fri_fold(sipp_ctx* ctx, const uint64_t* d_in, size_t len_in, uint32_t arity_bits, gl::E2 beta, uint64_t* d_out);
// one entry of the fused query-phase gather (sipp_k_gather_tasks): type 0 = oracle row (a = column stride, b = columns),
// 1 = Merkle siblings (b = log2 leaves, c = siblings, d = index shift), 2 = FRI leaf (a = values per component, b = shift, c = arity bits)
struct QueryGatherTask {
    const uint64_t* src;
    uint64_t* out;
    uint64_t a;
    uint32_t type, b, c, d;
};
int sipp_k_gather_tasks(sipp_ctx* ctx, const QueryGatherTask* d_tasks, uint32_t n_tasks, const uint32_t* d_idx, uint32_t nq);
// poseidon.hip
// leaf k = the 2^arity_bits consecutive (leaf-order) extension values [k 2^ab, (k + 1) 2^ab), flattened (c0, c1); hash_or_noop
int sipp_k_fri_leaves(sipp_ctx* ctx, const uint64_t* d_vals, size_t len, uint32_t arity_bits, uint64_t* d_digests);
// smallest w whose response has pow_bits leading zeros; response = word `resp_word` of permute(state with in_buf[0..n_in)
// and w at position n_in overwritten)
int sipp_k_pow_search(sipp_ctx* ctx, const uint64_t state[12], const uint64_t* in_buf, uint32_t n_in, uint32_t resp_word,
                      uint32_t pow_bits, uint64_t* witness);

// ---- host Poseidon + duplex challenger: host_challenger.hpp (shared with the host-only verifier, verify.cpp) ----

// ---- small host helpers of the provers ----------------------------------------------------------------------------
// out [count][2][3]: the limbs (gl::limbs3) of the two components of base^c, c < count -- the constant weights of the lazy
// combinations (prover.hip fri_combine_kernel and its kin).  Returns base^count.
inline gl::E2 sipp_pow_limbs(gl::E2 base, size_t count, uint32_t* out) {
    uint32_t(*o)[3] = reinterpret_cast<uint32_t(*)[3]>(out);
    gl::E2 x = gl::e2(1);
    for (size_t c = 0; c < count; c++) {
        gl::limbs3(o[2 * c], x.c0);
        gl::limbs3(o[2 * c + 1], x.c1);
        x = gl::mul(x, base);
    }
    return x;
}
// Exclusive prefix scan over the rows of [C][n] under a monoid of the field: one block of 1024 threads per challenge, every thread owns
// ceil(n / 1024) consecutive rows; out[i] = the combination of the rows before i, out[0] = the identity.  The outer prover's Z is the
// product instantiation (plonk.hip), the lookup argument's S the sum (lookup.hip).
struct ScanProduct {
    static constexpr uint64_t identity = 1;
    static __device__ uint64_t op(uint64_t a, uint64_t b) { return gl::mul(a, b); }
};
struct ScanSum {
    static constexpr uint64_t identity = 0;
    static __device__ uint64_t op(uint64_t a, uint64_t b) { return gl::add(a, b); }
};
template <typename Op>
static __global__ void __launch_bounds__(1024) sipp_scan_kernel(const uint64_t* tot, uint64_t* out, uint32_t log_n) {
    __shared__ uint64_t part[1024];
    const uint32_t n = 1u << log_n, c = blockIdx.x, T = blockDim.x;
    const uint32_t per = (n + T - 1) / T, lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
    const uint64_t* t = tot + (size_t)c * n;
    uint64_t* z = out + (size_t)c * n;
    uint64_t acc = Op::identity;
    for (uint32_t i = lo; i < hi; i++) acc = Op::op(acc, t[i]);
    part[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {          // Hillis-Steele inclusive scan of the 1024 partial results
        const uint64_t v = threadIdx.x >= d ? part[threadIdx.x - d] : Op::identity;
        __syncthreads();
        part[threadIdx.x] = Op::op(part[threadIdx.x], v);
        __syncthreads();
    }
    acc = threadIdx.x ? part[threadIdx.x - 1] : Op::identity;
    for (uint32_t i = lo; i < hi; i++) {
        z[i] = acc;
        acc = Op::op(acc, t[i]);
    }
}

// Z_H on the outer prover's quotient coset 7 <w_(n D)>, D = 2^log_d <= 64: x^n = 7^n w_D^(i mod D), so Z_H(x) = x^n - 1 takes D values;
// zh[d] and its inverse by coset index mod D (plonk.hip and lookup.hip hand them to their quotient kernels)
inline void sipp_coset_zh(uint32_t log_n, uint32_t log_d, uint64_t zh[64], uint64_t zh_inv[64]) {
    const uint64_t w_d = gl::root_of_unity(log_d);
    uint64_t f = gl::pow(gl::GEN, (uint64_t)1 << log_n);
    for (uint32_t d = 0; d < (1u << log_d); d++) {
        zh[d] = gl::sub(f, 1);
        zh_inv[d] = gl::inv(zh[d]);
        f = gl::mul(f, w_d);
    }
}
// natural-order radix-2 NTT on the host (the public-input polynomials, the value-periodic columns: sizes up to a few thousand):
// out[i] = sum_j a[j] w^(i j), w a primitive 2^log_n-th root (inverse: w^-1 and the factor 1 / n)
inline void sipp_host_ntt(uint64_t* a, uint32_t log_n, bool inverse) {
    const size_t n = (size_t)1 << log_n;
    for (size_t i = 0; i < n; i++) {
        const size_t j = gl::bitrev((uint32_t)i, log_n);
        if (i < j) std::swap(a[i], a[j]);
    }
    uint64_t root = gl::root_of_unity(log_n);
    if (inverse) root = gl::inv(root);
    for (uint32_t s = 1; s <= log_n; s++) {
        const size_t mlen = (size_t)1 << s, h = mlen >> 1;
        uint64_t wm = root;
        for (uint32_t k = s; k < log_n; k++) wm = gl::sqr(wm);
        for (size_t k = 0; k < n; k += mlen) {
            uint64_t w = 1;
            for (size_t j = 0; j < h; j++) {
                const uint64_t t = gl::mul(w, a[k + j + h]), u = a[k + j];
                a[k + j] = gl::add(u, t);
                a[k + j + h] = gl::sub(u, t);
                w = gl::mul(w, wm);
            }
        }
    }
    if (inverse) {
        const uint64_t ninv = gl::inv((uint64_t)n);
        for (size_t i = 0; i < n; i++) a[i] = gl::mul(a[i], ninv);
    }
}

// ---- the FRI core (fri.hip) ------------------------------------------------------------------------------------
struct FriOracleDev {
    const uint64_t* lde;    // [ncols][stride] leaf order (salt columns, if any, are the last ones)
    size_t stride;          // n << rate_bits
    uint32_t ncols;         // words per leaf
    const uint64_t* tree;   // levels back to back
};
// rounds of FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) for 2^degree_bits coefficients: fold while the
// polynomial is longer than the final one and the folded layer still has a cap
inline uint32_t sipp_fri_const_arity_rounds(uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t arity_bits,
                                            uint32_t final_poly_bits) {
    uint32_t rounds = 0;
    while (degree_bits > final_poly_bits && degree_bits + rate_bits - arity_bits >= cap_height && degree_bits >= arity_bits &&
           rounds < SIPP_FRI_MAX_ROUNDS) {
        rounds++;
        degree_bits -= arity_bits;
    }
    return rounds;
}
struct FriParamsDev {
    uint32_t rate_bits = 1, cap_height = 4, pow_bits = 16, num_queries = 84, pow_rule = 0;
    std::vector<uint32_t> arity_bits;   // FriParams::reduction_arity_bits
    uint32_t hasher = SIPP_HASH_POSEIDON;   // of the layer trees (the oracles' trees are the caller's); the challenger is Poseidon either way
    // the generic ABI's parameters (n_rounds beyond SIPP_FRI_MAX_ROUNDS is refused by the callers' checks, cut here)
    explicit FriParamsDev(const sipp_fri_params& p)
        : rate_bits(p.rate_bits), cap_height(p.cap_height), pow_bits(p.pow_bits), num_queries(p.num_queries), pow_rule(p.pow_rule),
          arity_bits(p.arity_bits, p.arity_bits + (p.n_rounds < SIPP_FRI_MAX_ROUNDS ? p.n_rounds : SIPP_FRI_MAX_ROUNDS)) {}
    // FriParams of a STARK over 2^degree_bits rows
    FriParamsDev(const sipp_stark_config& c, uint32_t degree_bits)
        : rate_bits(c.rate_bits), cap_height(c.cap_height), pow_bits(c.pow_bits), num_queries(c.num_queries), pow_rule(c.pow_rule),
          arity_bits(sipp_fri_const_arity_rounds(degree_bits, c.rate_bits, c.cap_height, c.arity_bits, c.final_poly_bits), c.arity_bits) {}
};
// u64 words of the section sipp_fri_prove_core appends (caps, final polynomial, witness, query rounds)
size_t sipp_fri_core_words(const FriParamsDev& p, uint32_t log_n, const uint32_t* leaf_words, int n_oracles);
// d_final: [2][n] extension coefficients (SoA) of the final polynomial, already multiplied by X
int sipp_fri_prove_core(sipp_ctx* ctx, const FriOracleDev* ors, int n_oracles, uint32_t log_n, const FriParamsDev& p,
                        uint64_t* d_final, host::Challenger& ch, uint64_t* pf, size_t& pos, size_t cap_total, size_t* final_len,
                        const std::function<void(const char*)>& tick);
