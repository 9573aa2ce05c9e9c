// sipp_amd/csrc/air_prog.hpp -- the one host reading of the gadget part of an AIR program (data/air_tables.h, written by
// tools/air_gen.py).  Host only, no HIP: trace.hip builds its gadget-offset and product-offset tables from it, prover.hip its
// segment table, tests/host/air_prog.cpp compares it with a second walk.
//
// Program format, in int64 words (tools/air_gen.py).  Gadgets come first, each one
//   1, sign_col, carry_base, carry_limbs, carry_bits, carry_offset, group | VEC q | np | np x (coef, VEC a, VEC b) | nl | nl x (coef, VEC a)
// with VEC = n_limbs, k, k x 5 words; then POLY ops up to prog_len, each one
//   2, n_mono | n_mono x (coef, k, k x 2 words)
#pragma once
#include <stdint.h>

#include <vector>

struct AirGadget {
    uint32_t off;                    // of its op word (1)
    int64_t group;                   // w[6]: the limbs of one constraint group
    int64_t np;                      // products
    std::vector<uint32_t> prod_off;  // np + 1 offsets: every product, then the word behind the last one
};

struct AirGadgets {
    std::vector<AirGadget> gadgets;
    uint32_t poly_off = 0;           // where the POLY ops begin (prog_len for a program without any)
};

static inline AirGadgets air_read_gadgets(const int64_t* prog, int64_t prog_len) {
    AirGadgets r;
    const int64_t* w = prog;
    const int64_t* end = prog + prog_len;
    auto vec = [&] { w += 2 + 5 * w[1]; };
    while (w < end && w[0] == 1) {
        AirGadget g;
        g.off = (uint32_t)(w - prog);
        g.group = w[6];
        w += 7;
        vec();
        g.np = *w++;
        for (int64_t p = 0; p < g.np; p++) {
            g.prod_off.push_back((uint32_t)(w - prog));
            w += 1;
            vec();
            vec();
        }
        g.prod_off.push_back((uint32_t)(w - prog));
        const int64_t nl = *w++;
        for (int64_t p = 0; p < nl; p++) {
            w += 1;
            vec();
        }
        r.gadgets.push_back(g);
    }
    r.poly_off = (uint32_t)(w - prog);
    return r;
}
