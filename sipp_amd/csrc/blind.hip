// sipp_amd/csrc/blind.hip -- the randomness of a zero-knowledge outer proof, drawn on the device from a seed: the salt columns of the
// wires, Z / partial-products and quotient oracles (plonky2's PolynomialBatch salt under FriParams::hiding) and the cells of the blinding
// rows (SIPP_GEN_RANDOM).  ONE random function, fixed in include/sipp_hip.h and read a second time in tests/_blinding_cases.py:
//   block(seed[4], counter, stream, index) = the first 8 words of hash_n_to_m_no_pad([seed0..3, counter, stream, index], 8)
//                                          = one permutation of [seed0, seed1, seed2, seed3, counter, stream, index, 0, 0, 0, 0, 0]
// Salt: leaf j of stream s (LEAF order, the order of d_lde) takes words 4 (j & 1) .. + 3 of block(seed, counter, s, j >> 1).
// Blinding rows: wire w of table row r takes word w & 7 of block(seed, counter, 0, r 2^9 + (w >> 3)).
//
// Kernels: one lane per permutation, the one-state-per-lane VALU form of poseidon.hpp (no matrix pipe: these launches are thin next to
// leaf hashing and need no whole waves).  The salt kernel has one lane per leaf PAIR: it writes 16 bytes into each of the four salt
// columns, consecutive lanes consecutive 16-byte pieces.
#include <mutex>

#include "ctx.hpp"
#ifndef GLL_T
#define GLL_T 140      // the product block's register window (gl_lazy.hpp), as in poseidon.hip
#endif
#include "poseidon.hpp"
#include "prover.hpp"

namespace {

constexpr uint32_t MAX_SALT_TARGETS = 3;

struct BlindKey {
    uint64_t seed[4], counter;
};

__device__ __forceinline__ void block(const BlindKey& k, uint64_t stream, uint64_t index, uint64_t s[12]) {
    s[0] = k.seed[0]; s[1] = k.seed[1]; s[2] = k.seed[2]; s[3] = k.seed[3];
    s[4] = k.counter; s[5] = stream; s[6] = index;
#pragma unroll
    for (int i = 7; i < 12; i++) s[i] = 0;
    poseidon::permute(s);      // canonical outputs
}

struct SaltArgs {
    BlindKey key;
    uint64_t* base[MAX_SALT_TARGETS];      // the first salt column of each oracle: d_lde + ncols * leaves (16-byte aligned)
    uint32_t stream[MAX_SALT_TARGETS];
    uint64_t leaves;                       // per column, even
};

__global__ void __launch_bounds__(256) salt_columns_kernel(SaltArgs a) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;      // leaf pair
    if (b >= (a.leaves >> 1)) return;
    uint64_t s[12];
    block(a.key, a.stream[blockIdx.y], b, s);
    uint64_t* out = a.base[blockIdx.y] + 2 * b;
#pragma unroll
    for (int k = 0; k < 4; k++) *reinterpret_cast<ulonglong2*>(out + (size_t)k * a.leaves) = make_ulonglong2(s[k], s[4 + k]);
}

struct RowsArgs {
    BlindKey key;
    uint64_t* wires;           // [num_wires][n]
    const uint64_t* consts;    // [num_constants][n]
    uint32_t n, selector_index, row, w0, w1, chunk0;      // wires w0 .. w1 - 1; chunk0 = w0 >> 3
};

// one lane per (table row, eight wires): a row that does not hold the generator leaves at once
__global__ void __launch_bounds__(256) blind_rows_kernel(RowsArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    if (a.consts[(size_t)a.selector_index * a.n + i] != a.row) return;
    const uint32_t c = a.chunk0 + blockIdx.y;
    uint64_t s[12];
    block(a.key, 0, ((uint64_t)i << 9) + c, s);
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const uint32_t w = 8 * c + q;
        if (w >= a.w0 && w < a.w1) a.wires[(size_t)w * a.n + i] = s[q];
    }
}

// this translation unit's copies of the tables the VALU permutation reads, once per device (a blocking copy, complete before any launch)
int upload_tables(sipp_ctx* ctx) {
    static std::mutex mu;
    static bool done[64] = {false};
    std::lock_guard<std::mutex> lk(mu);
    const int dev = ctx->device & 63;
    if (done[dev]) return SIPP_OK;
    SIPP_CHECK_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(poseidon::c_rc), SIPP_POSEIDON_RC, sizeof(SIPP_POSEIDON_RC)));
    SIPP_CHECK_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(poseidon::c_fast_scalar), SIPP_POSEIDON_FAST_SCALAR, sizeof(SIPP_POSEIDON_FAST_SCALAR)));
    SIPP_CHECK_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(poseidon::c_blk3), SIPP_POSEIDON_BLK3, sizeof(SIPP_POSEIDON_BLK3)));
    SIPP_CHECK_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(poseidon::c_comb3), SIPP_POSEIDON_COMB3, sizeof(SIPP_POSEIDON_COMB3)));
    SIPP_CHECK_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(poseidon::c_comb_c), SIPP_POSEIDON_COMB_C, sizeof(SIPP_POSEIDON_COMB_C)));
    done[dev] = true;
    return SIPP_OK;
}

BlindKey key_of(const sipp_blinding& b) { return BlindKey{{b.seed[0], b.seed[1], b.seed[2], b.seed[3]}, b.counter}; }

}  // namespace

int sipp_blind_check(sipp_ctx* ctx, const sipp_blinding* b) {
    if (!b) return sipp_fail(ctx, SIPP_E_BADARG, "blinding: no seed");
    for (int q = 0; q < 4; q++)
        if (b->seed[q] >= gl::P) return sipp_fail(ctx, SIPP_E_BADARG, "blinding: a seed word is not a canonical field element");
    if (b->counter >= gl::P) return sipp_fail(ctx, SIPP_E_BADARG, "blinding: the counter is not a canonical field element");
    return SIPP_OK;
}

int sipp_blind_salt_launch(sipp_ctx* ctx, const sipp_blinding& b, uint64_t* const* bases, const uint32_t* streams, uint32_t n_targets,
                           uint32_t log_m) {
    if (n_targets == 0) return SIPP_OK;
    if (n_targets > MAX_SALT_TARGETS || log_m < 1 || log_m > 30) return sipp_fail(ctx, SIPP_E_BADARG, "blinding: bad salt launch");
    SIPP_TRY(upload_tables(ctx));
    SaltArgs a;
    a.key = key_of(b);
    a.leaves = (uint64_t)1 << log_m;
    for (uint32_t t = 0; t < MAX_SALT_TARGETS; t++) {
        a.base[t] = bases[t < n_targets ? t : 0];
        a.stream[t] = streams[t < n_targets ? t : 0];
        if ((uintptr_t)a.base[t] & 15) return sipp_fail(ctx, SIPP_E_BADARG, "blinding: the salt columns must start at a 16-byte boundary");
    }
    const uint64_t pairs = a.leaves >> 1;
    ProfScope ps(ctx, "blind_salt");
    hipLaunchKernelGGL(salt_columns_kernel, dim3((unsigned)((pairs + 255) / 256), n_targets), dim3(256), 0, ctx->stream, a);
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    return SIPP_OK;
}

int sipp_blind_rows_launch(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, const sipp_plonk_generator& g,
                           const sipp_blinding& b) {
    if (g.p[1] == 0) return SIPP_OK;
    SIPP_TRY(upload_tables(ctx));
    RowsArgs a;
    a.key = key_of(b);
    a.wires = d_wires; a.consts = d_constants; a.n = 1u << log_n; a.selector_index = g.selector_index; a.row = g.row;
    a.w0 = g.p[0]; a.w1 = g.p[0] + g.p[1]; a.chunk0 = a.w0 >> 3;
    const uint32_t chunks = ((a.w1 - 1) >> 3) - a.chunk0 + 1;
    ProfScope ps(ctx, "blind_rows");
    hipLaunchKernelGGL(blind_rows_kernel, dim3((a.n + 255) / 256, chunks), dim3(256), 0, ctx->stream, a);
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    return SIPP_OK;
}

extern "C" int sipp_blind_salt(sipp_ctx* ctx, uint64_t* d_lde, uint32_t ncols, uint32_t log_m, const uint64_t* blind_words, uint32_t stream) {
    if (!ctx) return SIPP_E_BADARG;
    const BlindArg arg(blind_words);
    const sipp_blinding* blind = arg.p;
    if (!d_lde || !ncols || log_m < 1 || log_m > 30 || stream < 1 || stream > 3)
        return sipp_fail(ctx, SIPP_E_BADARG, "blind_salt: null buffer, no column, log_m outside 1 .. 30 or a stream outside 1 .. 3");
    SIPP_TRY(sipp_blind_check(ctx, blind));
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t* base = d_lde + ((size_t)ncols << log_m);
    SIPP_TRY(sipp_blind_salt_launch(ctx, *blind, &base, &stream, 1, log_m));
    return sipp_sync(ctx);
}
