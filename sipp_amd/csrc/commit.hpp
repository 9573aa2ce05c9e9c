// sipp_amd/csrc/commit.hpp -- committing a PolynomialBatch (plonky2 fri/oracle.rs from_values / from_coeffs): values -> coefficients
// -> coset LDE -> leaves (Poseidon, or Keccak where the caller names it) -> Merkle levels -> cap.  The ONE host path of the STARK prover (stark.hip), the building-block
// ABI (api.hip) and the generic commitments of the outer prover and CircuitData (fri.hip sipp_commit_batch_ex).  The callers keep what
// is theirs: argument checks, hipSetDevice, and whether they synchronise after a failure.
#pragma once
#include "ctx.hpp"

// what a commitment needs beyond the ctx: the STARK prover and the building blocks take the first two from ctx->cfg, the generic ABI
// from its arguments
struct CommitParams {
    uint32_t rate_bits, cap_height;
    const uint64_t* d_salt = nullptr;   // n_salt columns of n << rate_bits words in natural LDE order, hashed behind the polynomials'
    uint32_t n_salt = 0;
    // the n_salt columns already sit behind the polynomial columns of d_lde, in LEAF order (blind.hip filled them): d_salt is not read
    bool salt_in_place = false;
    uint32_t hasher = SIPP_HASH_POSEIDON;   // the tree hasher (keccak.hip: sipp_k_tree_leaves / sipp_k_tree_levels); 0 = the Poseidon launches
};

// u64 words of a Merkle tree over 2^log_leaves leaves, levels back to back: 2 * leaves * 4
inline size_t tree_words(uint32_t log_leaves) { return (size_t)8 << log_leaves; }

// d_in [ncols][n] natural order (values, or with from_coeffs coefficients) -> d_coeffs [ncols][n] natural -> d_lde [ncols][n << rate_bits]
// in leaf order.  d_in == d_coeffs is allowed either way.  Launches only.
int commit_lde(sipp_ctx* ctx, const uint64_t* d_in, bool from_coeffs, uint64_t* d_coeffs, uint64_t* d_lde, size_t ncols, uint32_t log_n,
               uint32_t rate_bits);
// commit_lde, the salt columns behind the LDE's, leaves and levels into d_tree (tree_words(log_n + rate_bits)).  Launches only: the
// host may work while they run (prove_impl does) and collects the cap with read_cap.
int commit_launch(sipp_ctx* ctx, const CommitParams& cp, const uint64_t* d_in, bool from_coeffs, uint64_t* d_coeffs, uint64_t* d_lde,
                  uint64_t* d_tree, size_t ncols, uint32_t log_n);
// the 4 << min(cap_height, log_leaves) words of the cap level to the host; returns with the stream synchronised
int read_cap(sipp_ctx* ctx, const uint64_t* d_tree, uint32_t log_leaves, uint32_t cap_height, uint64_t* cap_host);
// commit_launch + read_cap
int commit_batch(sipp_ctx* ctx, const CommitParams& cp, const uint64_t* d_in, bool from_coeffs, uint64_t* d_coeffs, uint64_t* d_lde,
                 uint64_t* d_tree, size_t ncols, uint32_t log_n, uint64_t* cap_host);
