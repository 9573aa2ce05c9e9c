// sipp_amd/csrc/commit.hip -- see commit.hpp.  Host code only: the kernels are ntt.hip's, ntt_tree.hip's, poseidon.hip's and keccak.hip's.
#include <algorithm>

#include "commit.hpp"

int commit_lde(sipp_ctx* ctx, const uint64_t* d_in, bool from_coeffs, uint64_t* d_coeffs, uint64_t* d_lde, size_t ncols, uint32_t log_n,
               uint32_t rate_bits) {
    const size_t n = (size_t)1 << log_n;
    if (!from_coeffs) {
        // the fused transform first: coefficients and LDE in one chain.  It answers SIPP_E_UNSUPPORTED for the shapes it does not
        // cover (short columns, d_coeffs aliasing d_in on a long column) ...
        const int rc = sipp_lde_from_values(ctx, d_in, d_coeffs, d_lde, ncols, log_n, rate_bits);
        if (rc != SIPP_E_UNSUPPORTED) return rc;
        // ... and those go pass by pass: bit-reversal copy, inverse DIT, coset DIF.  The copy works out of place, so an aliased input
        // moves to a temporary first (handed back on every exit path; the stream is ordered, so later users of the block wait)
        ArenaScope scope(ctx);
        const uint64_t* src = d_in;
        if (d_in == d_coeffs) {
            uint64_t* tmp = arena_alloc_t<uint64_t>(ctx, n * ncols);
            if (!tmp) return SIPP_E_NOMEM;
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(tmp, d_in, n * ncols * 8, hipMemcpyDeviceToDevice, ctx->stream));
            src = tmp;
        }
        SIPP_TRY(sipp_bitrev_cols(ctx, src, n, d_coeffs, n, log_n, ncols));
        SIPP_TRY(sipp_ntt_dit(ctx, d_coeffs, n, log_n, ncols, /*inverse=*/true, NttDiag{}));
        return sipp_ntt_dif(ctx, d_coeffs, n, log_n, d_lde, n << rate_bits, log_n + rate_bits, ncols, false, NttDiag{gl::GEN, 0});
    }
    if (d_in != d_coeffs) SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_coeffs, d_in, ncols * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    const int rc = sipp_lde_from_coeffs(ctx, d_coeffs, d_lde, ncols, log_n, rate_bits);
    if (rc != SIPP_E_UNSUPPORTED) return rc;
    return sipp_ntt_dif(ctx, d_coeffs, n, log_n, d_lde, n << rate_bits, log_n + rate_bits, ncols, false, NttDiag{gl::GEN, 0});
}

int commit_launch(sipp_ctx* ctx, const CommitParams& cp, const uint64_t* d_in, bool from_coeffs, uint64_t* d_coeffs, uint64_t* d_lde,
                  uint64_t* d_tree, size_t ncols, uint32_t log_n) {
    const uint32_t log_m = log_n + cp.rate_bits;
    const size_t m = (size_t)1 << log_m;
    SIPP_TRY(commit_lde(ctx, d_in, from_coeffs, d_coeffs, d_lde, ncols, log_n, cp.rate_bits));
    // salt columns: natural LDE order in, leaf order (= bit-reversed rows) behind the polynomial columns -- unless they are there already
    if (cp.n_salt && !cp.salt_in_place) SIPP_TRY(sipp_bitrev_cols(ctx, cp.d_salt, m, d_lde + ncols * m, m, log_m, cp.n_salt));
    SIPP_TRY(sipp_k_tree_leaves(ctx, cp.hasher, d_lde, m, ncols + cp.n_salt, log_m, d_tree));
    return sipp_k_tree_levels(ctx, cp.hasher, d_tree, log_m, cp.cap_height);
}

int read_cap(sipp_ctx* ctx, const uint64_t* d_tree, uint32_t log_leaves, uint32_t cap_height, uint64_t* cap_host) {
    const uint32_t ch = std::min(cap_height, log_leaves);
    uint64_t off = 0;   // nodes of the levels below the cap's
    for (uint32_t l = 0; l < log_leaves - ch; l++) off += (uint64_t)1 << (log_leaves - l);
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(cap_host, d_tree + 4 * off, ((size_t)4 << ch) * 8, hipMemcpyDeviceToHost, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SIPP_OK;
}

int commit_batch(sipp_ctx* ctx, const CommitParams& cp, const uint64_t* d_in, bool from_coeffs, uint64_t* d_coeffs, uint64_t* d_lde,
                 uint64_t* d_tree, size_t ncols, uint32_t log_n, uint64_t* cap_host) {
    SIPP_TRY(commit_launch(ctx, cp, d_in, from_coeffs, d_coeffs, d_lde, d_tree, ncols, log_n));
    return read_cap(ctx, d_tree, log_n + cp.rate_bits, cp.cap_height, cap_host);
}
