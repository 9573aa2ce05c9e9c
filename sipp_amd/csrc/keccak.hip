// sipp_amd/csrc/keccak.hip -- Merkle trees hashed with Keccak-256 truncated to 25 bytes (plonky2's KeccakGoldilocksConfig: KeccakHash<25>
// for leaves, nodes and caps; the challenger stays Poseidon).  One leaf / node per lane; the permutation and the packing of a digest
// into four words are host_keccak.hpp's, the same text the host verifier runs.
//
// Layouts are poseidon.hip's: the LDE column-major [col][leaf] in leaf order (64 lanes read 64 consecutive u64 of one column per load),
// digests [node][4] u64, the tree's levels back to back.  A hashed state is 25 lanes of 64 bits = 50 VGPRs; no LDS, no matrix pipe, so
// a lane past the end simply leaves.
#include <algorithm>

#include "ctx.hpp"
#include "host_keccak.hpp"
#include "prover.hpp"

namespace {

// hash_or_noop(leaf): 17 columns absorbed per permutation, every word reduced to its canonical form first (Poseidon does not care
// about the representative, Keccak hashes bytes); at most three columns: the 24 bytes re-cut into 7-byte words, nothing hashed
__global__ void __launch_bounds__(256) keccak_leaves_kernel(const uint64_t* __restrict__ lde, size_t col_stride, uint32_t ncols,
                                                           uint64_t n_leaves, uint64_t* __restrict__ digests) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_leaves) return;
    const uint64_t* p = lde + j;
    uint64_t out[4];
    keccak::hash_or_noop_with(ncols, [p, col_stride](uint32_t c) { return p[(size_t)c * col_stride]; }, out);
    uint64_t* d = digests + 4 * j;
    d[0] = out[0];
    d[1] = out[1];
    d[2] = out[2];
    d[3] = out[3];
}

// FRI layer leaves: leaf k = 2^ab consecutive (leaf-order) extension values, flattened (c0, c1) as in poseidon.hip's fri_leaves_*:
// 4, 8, 16 or 32 words, all above 25 bytes, so every arity is hashed (arity 2 is a no-op under Poseidon)
__global__ void __launch_bounds__(256) keccak_fri_leaves_kernel(const uint64_t* __restrict__ vals, uint64_t len, uint32_t ab,
                                                               uint64_t* __restrict__ digests) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (len >> ab)) return;
    const uint64_t* c0 = vals + (k << ab);
    const uint64_t* c1 = vals + len + (k << ab);
    uint64_t out[4];
    keccak::hash_or_noop_with(2u << ab, [c0, c1](uint32_t e) { return (e & 1) ? c1[e >> 1] : c0[e >> 1]; }, out);
    uint64_t* d = digests + 4 * k;
    d[0] = out[0];
    d[1] = out[1];
    d[2] = out[2];
    d[3] = out[3];
}

// Merkle levels, poseidon.hip's subtree form: block b owns the 2^lw nodes [b 2^lw, (b + 1) 2^lw) of level `level0` and climbs nlev
// levels inside them; a level it produces goes to the tree (queries need every level's siblings) and is read back by the same block
// behind a barrier.  One node per lane: two digests unpacked to 50 bytes, one permutation, 25 bytes repacked.
__global__ void __launch_bounds__(256) keccak_merkle_subtree_kernel(uint64_t* tree, uint32_t log_leaves, uint32_t level0, uint32_t lw,
                                                                   uint32_t nlev) {
    uint64_t off = 0;
    for (uint32_t l = 0; l < level0; l++) off += (uint64_t)1 << (log_leaves - l);
    uint64_t n_level = (uint64_t)1 << (log_leaves - level0);   // nodes of the current level in the whole tree
    uint64_t first = (uint64_t)blockIdx.x << lw;               // this block's first node on the current level
    uint32_t cnt = 1u << lw;                                    // this block's nodes on the current level
    for (uint32_t s = 0; s < nlev; s++) {
        const uint64_t* child = tree + 4 * (off + first);
        uint64_t* parent = tree + 4 * (off + n_level + (first >> 1));
        cnt >>= 1;
#pragma unroll 1
        for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
            const uint64_t* c = child + 8 * (uint64_t)i;
            uint64_t l[4], r[4], out[4];
#pragma unroll
            for (int k = 0; k < 4; k++) l[k] = c[k], r[k] = c[4 + k];
            keccak::two_to_one(l, r, out);
            uint64_t* d = parent + 4 * (uint64_t)i;
            d[0] = out[0];
            d[1] = out[1];
            d[2] = out[2];
            d[3] = out[3];
        }
        __syncthreads();
        off += n_level;
        n_level >>= 1;
        first >>= 1;
    }
}

// one lane per leaf, and a HIP launch holds fewer than 2^32 lanes: 2^31 leaves at the most (the level launches take 2^11 nodes a block
// of 256 lanes and stay below that); the launchers refuse more where the grid would otherwise wrap or the launch fail
constexpr uint32_t KECCAK_MAX_LOG_LEAVES = 31;

}  // namespace

int sipp_k_keccak_leaves(sipp_ctx* ctx, const uint64_t* d_lde, size_t col_stride, size_t ncols, uint32_t log_leaves, uint64_t* d_digests) {
    if (ncols == 0 || ncols > 0xffffffffull) return sipp_fail(ctx, SIPP_E_BADARG, "keccak_leaves: bad ncols");
    if (log_leaves > KECCAK_MAX_LOG_LEAVES) return sipp_fail(ctx, SIPP_E_BADARG, "keccak_leaves: more leaves than one launch holds (2^31)");
    const uint64_t n = (uint64_t)1 << log_leaves;
    ProfScope ps(ctx, ncols <= 3 ? "keccak_leaves_noop" : "keccak_leaves");
    hipLaunchKernelGGL(keccak_leaves_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_lde, col_stride, (uint32_t)ncols,
                       n, d_digests);
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    return SIPP_OK;
}

int sipp_k_keccak_fri_leaves(sipp_ctx* ctx, const uint64_t* d_vals, size_t len, uint32_t arity_bits, uint64_t* d_digests) {
    if (arity_bits < 1 || arity_bits > 4) return sipp_fail(ctx, SIPP_E_UNSUPPORTED, "fri_leaves: arity must be 2, 4, 8 or 16");
    const uint64_t nl = len >> arity_bits;
    if (nl == 0) return sipp_fail(ctx, SIPP_E_BADARG, "fri_leaves: fewer values than one leaf");
    if (nl > ((uint64_t)1 << KECCAK_MAX_LOG_LEAVES)) return sipp_fail(ctx, SIPP_E_BADARG, "fri_leaves: more leaves than one launch holds (2^31)");
    ProfScope ps(ctx, "keccak_fri_leaves");
    hipLaunchKernelGGL(keccak_fri_leaves_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, ctx->stream, d_vals, (uint64_t)len,
                       arity_bits, d_digests);
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    return SIPP_OK;
}

int sipp_k_keccak_merkle_levels(sipp_ctx* ctx, uint64_t* d_tree, uint32_t log_leaves, uint32_t cap_height) {
    if (log_leaves > KECCAK_MAX_LOG_LEAVES) return sipp_fail(ctx, SIPP_E_BADARG, "keccak_merkle_levels: more leaves than one launch holds (2^31)");
    if (cap_height > log_leaves) cap_height = log_leaves;
    const uint32_t top = log_leaves - cap_height;   // levels to produce
    uint32_t level = 0;
    while (level < top) {
        const uint32_t log_nodes = log_leaves - level;
        // wide levels (more than 2^11 nodes): blocks of 2^11 nodes climb three levels -- 1024, 512, 256 parents, a parent for every
        // lane on each; from 2^11 nodes down ONE block climbs to the cap (few nodes, launch-bound: one launch instead of eleven)
        const uint32_t lw = log_nodes > 11 ? 11 : log_nodes;
        const uint32_t nlev = log_nodes > 11 ? std::min(3u, top - level) : top - level;
        ProfScope ps(ctx, "keccak_merkle_subtree");
        hipLaunchKernelGGL(keccak_merkle_subtree_kernel, dim3(1u << (log_nodes - lw)), dim3(256), 0, ctx->stream, d_tree, log_leaves, level,
                           lw, nlev);
        SIPP_CHECK_HIP(ctx, hipGetLastError());
        level += nlev;
    }
    return SIPP_OK;
}

// ---- the hasher as an argument: 0 = the Poseidon kernels, launched exactly as before; 1 = the kernels above ----
int sipp_k_tree_leaves(sipp_ctx* ctx, uint32_t hasher, const uint64_t* d_lde, size_t col_stride, size_t ncols, uint32_t log_leaves,
                       uint64_t* d_digests) {
    if (hasher == SIPP_HASH_POSEIDON) return sipp_k_poseidon_leaves(ctx, d_lde, col_stride, ncols, log_leaves, d_digests);
    SIPP_TRY(sipp_hasher_check(ctx, hasher));
    return sipp_k_keccak_leaves(ctx, d_lde, col_stride, ncols, log_leaves, d_digests);
}
int sipp_k_tree_fri_leaves(sipp_ctx* ctx, uint32_t hasher, const uint64_t* d_vals, size_t len, uint32_t arity_bits, uint64_t* d_digests) {
    if (hasher == SIPP_HASH_POSEIDON) return sipp_k_fri_leaves(ctx, d_vals, len, arity_bits, d_digests);
    SIPP_TRY(sipp_hasher_check(ctx, hasher));
    return sipp_k_keccak_fri_leaves(ctx, d_vals, len, arity_bits, d_digests);
}
int sipp_k_tree_levels(sipp_ctx* ctx, uint32_t hasher, uint64_t* d_tree, uint32_t log_leaves, uint32_t cap_height) {
    if (hasher == SIPP_HASH_POSEIDON) return sipp_k_merkle_levels(ctx, d_tree, log_leaves, cap_height);
    SIPP_TRY(sipp_hasher_check(ctx, hasher));
    return sipp_k_keccak_merkle_levels(ctx, d_tree, log_leaves, cap_height);
}
