// sipp_amd/csrc/host_challenger.hpp -- the host-side Fiat-Shamir challenger (plonky2 iop/challenger.rs as recalled)
// over the host Poseidon permutation: plain C++, no HIP.  Used by the provers (stark.hip, fri.hip, plonk.hip) and by the host-only
// verifier (verify.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sipp_hip.h"
#include "gl.hpp"
#include "host_poseidon.hpp"

namespace host {

// The permutation itself lives in host_poseidon.cpp (portable scalar and AVX-512 forms, bit-identical, chosen at load time):
// observing the ~32 k opening words of the widest STARK is ~4 k sequential permutations on the proof's critical path.
// Checked against the device kernel by every proof parity test and against the CPU oracle by tests/test_abi.py.

struct Challenger {
    uint64_t state[12] = {0};
    uint64_t in_buf[8];
    uint32_t n_in = 0;
    uint64_t out_buf[8];
    uint32_t n_out = 0;
    void duplex() {
        for (uint32_t i = 0; i < n_in; i++) state[i] = in_buf[i];
        n_in = 0;
        poseidon_permute(state);
        for (int i = 0; i < 8; i++) out_buf[i] = state[i];
        n_out = 8;
    }
    void observe(uint64_t e) {
        n_out = 0;
        in_buf[n_in++] = e;
        if (n_in == 8) duplex();
    }
    void observe_many(const uint64_t* e, size_t n) {
        for (size_t i = 0; i < n; i++) observe(e[i]);
    }
    uint64_t get() {
        if (n_in != 0 || n_out == 0) duplex();
        return out_buf[--n_out];
    }
    // hash_n_to_hash_no_pad (overwrite-mode sponge, rate 8) and two_to_one, for the statement binding of stark.hip
    static void hash_no_pad(const uint64_t* in, size_t n, uint64_t out[4]) {
        uint64_t s[12] = {0};
        for (size_t i = 0; i < n; i += 8) {
            for (size_t k = 0; k < 8 && i + k < n; k++) s[k] = in[i + k];
            poseidon_permute(s);
        }
        for (int k = 0; k < 4; k++) out[k] = s[k];
    }
    static void two_to_one(const uint64_t l[4], const uint64_t r[4], uint64_t out[4]) {
        uint64_t s[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
        poseidon_permute(s);
        for (int k = 0; k < 4; k++) out[k] = s[k];
    }
    gl::E2 get_ext() {
        gl::E2 r;
        r.c0 = get();
        r.c1 = get();
        return r;
    }
    // the transcript as the plain data of the C ABI, both ways (a plain copy: the callers check n_in / n_out of foreign states)
    explicit Challenger(const sipp_challenger& c) : n_in((uint32_t)c.n_in), n_out((uint32_t)c.n_out) {
        memcpy(state, c.state, sizeof state);
        memcpy(in_buf, c.in_buf, sizeof in_buf);
        memcpy(out_buf, c.out_buf, sizeof out_buf);
    }
    Challenger() = default;
    void store(sipp_challenger* c) const {
        memcpy(c->state, state, sizeof state);
        memcpy(c->in_buf, in_buf, sizeof in_buf);
        memcpy(c->out_buf, out_buf, sizeof out_buf);
        c->n_in = n_in;
        c->n_out = n_out;
    }
};

}  // namespace host
