// sipp_amd/csrc/host_tree_hash.hpp -- the two functions a Merkle path is climbed with on the host, by tree hasher: Poseidon
// (host_challenger.hpp: at most four elements are the digest themselves, zero padded) or Keccak-256 truncated to 25 bytes
// (host_keccak.hpp).  ONE text for the verifier (verify.cpp) and the C ABI's test surface (api.hip sipp_host_merkle_hash).
#pragma once
#include <string.h>

#include "../../include/sipp_hip.h"
#include "host_challenger.hpp"
#include "host_keccak.hpp"

namespace host {

inline void tree_hash_or_noop(uint32_t hasher, const uint64_t* leaf, size_t leaf_len, uint64_t out[4]) {
    if (hasher == SIPP_HASH_KECCAK25) {
        keccak::hash_or_noop(leaf, leaf_len, out);
        return;
    }
    out[0] = out[1] = out[2] = out[3] = 0;
    if (leaf_len == 0) return;
    if (leaf_len <= 4) memcpy(out, leaf, leaf_len * 8);
    else Challenger::hash_no_pad(leaf, leaf_len, out);
}

inline void tree_two_to_one(uint32_t hasher, const uint64_t* l, const uint64_t* r, uint64_t out[4]) {
    if (hasher == SIPP_HASH_KECCAK25) keccak::two_to_one(l, r, out);
    else Challenger::two_to_one(l, r, out);
}

}  // namespace host
