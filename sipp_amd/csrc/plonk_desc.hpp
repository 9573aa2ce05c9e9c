// sipp_amd/csrc/plonk_desc.hpp -- the outer prover's three DESCRIPTIONS, read once: sipp_plonk_params, the gate set sipp_plonk_circuit and
// the eight-word lookup description (include/sipp_hip.h).  Host only, header only, plain C++17: the prover (plonk.hip, lookup.hip,
// circuit_data.hip) and the host-only verifier (verify.cpp) both rest on these readings, so nothing here knows of a ctx, of an error
// message or of the device.  Every function returns a REASON; the callers map it to their status and message (the prover) or to a
// refusing stage (the verifier).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/sipp_hip.h"

namespace plonk_desc {

constexpr uint32_t MAX_CH = 8, MAX_CHUNKS = 32, MAX_SLOTS = 128;

// ---- sipp_plonk_params ---------------------------------------------------------------------------------------------------------------
enum class Params { ok, bad_argument, chunk_size, counts };      // chunk_size, counts: sizes this build does not serve
// what a caller needs beyond the chunk size and the challenges: ROUTED = the permutation argument runs (num_routed_wires != 0);
// CHUNK_CAP = its kernels run (at most 32 chunks of routed wires).  The lookup columns need neither, the verifier the first alone.
enum : unsigned { ROUTED = 1, CHUNK_CAP = 2 };
// fills log_d = log2(max_degree) and m = the chunks of routed wires
inline Params params_check(const sipp_plonk_params* p, uint32_t log_n, unsigned need, uint32_t* log_d, uint32_t* m) {
    if (!p || ((need & ROUTED) && p->num_routed_wires == 0) || p->num_challenges == 0 || log_n < 1 || log_n > 24) return Params::bad_argument;
    const uint32_t D = p->max_degree;
    if (D < 2 || D > 64 || (D & (D - 1))) return Params::chunk_size;
    const uint32_t chunks = (p->num_routed_wires + D - 1) / D;
    if (((need & CHUNK_CAP) && chunks > MAX_CHUNKS) || p->num_challenges > MAX_CH) return Params::counts;
    uint32_t ld = 0;
    while ((1u << ld) < D) ld++;
    *log_d = ld;
    *m = chunks;
    return Params::ok;
}

// ---- the size caps of a circuit: what the prover's buffers and launch shapes are sized for --------------------------------------------
inline bool sizes_within_caps(uint32_t num_wires, uint32_t num_constants) { return num_wires <= 4096 && num_constants <= 1024; }

// ---- the lookup description ------------------------------------------------------------------------------------------------------------
struct Lookup {
    uint32_t q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab, tag_const0;
    bool empty() const { return n_look == 0 && n_tab == 0; }
    bool tagged() const { return tag_const0 != 0; }
    // groups of at most D slots: one S / U column each per challenge
    uint32_t Jl(uint32_t D) const { return (n_look + D - 1) / D; }
    uint32_t Jt(uint32_t D) const { return (n_tab + D - 1) / D; }
    uint32_t columns(uint32_t D, uint32_t C) const { return C * (Jl(D) + Jt(D)); }
};
inline Lookup lookup_of(const uint32_t* w) { return Lookup{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]}; }
// word q of the description, as a proof's header carries it
inline uint32_t lookup_word(const Lookup& l, int q) {
    const uint32_t w[8] = {l.q_look, l.look_wire0, l.n_look, l.q_tab, l.tab_const0, l.tab_mult0, l.n_tab, l.tag_const0};
    return w[q];
}

// the refusals of include/sipp_hip.h, in its order: sizes the build does not serve, then a description that does not fit the circuit
// (an empty description passes)
enum class LookupReason { ok, too_many_slots, empty_with_tag, one_sided, circuit_sizes, column_outside, marker_is_selector, tag_columns };
inline LookupReason lookup_check(const Lookup& l, uint32_t num_wires, uint32_t num_constants, uint32_t num_selectors) {
    if (l.n_look > MAX_SLOTS || l.n_tab > MAX_SLOTS) return LookupReason::too_many_slots;
    if (l.empty()) return l.tagged() ? LookupReason::empty_with_tag : LookupReason::ok;
    if (l.n_look == 0 || l.n_tab == 0) return LookupReason::one_sided;
    if (!sizes_within_caps(num_wires, num_constants) || num_selectors > num_constants) return LookupReason::circuit_sizes;
    // (every sum below stays far inside 32 bits: the counts are <= 128, the columns are checked first)
    if (l.q_look >= num_constants || l.q_tab >= num_constants || l.look_wire0 >= num_wires || l.look_wire0 + 2 * l.n_look > num_wires ||
        l.tab_const0 >= num_constants || l.tab_const0 + 2 * l.n_tab > num_constants || l.tab_mult0 >= num_wires ||
        l.tab_mult0 + l.n_tab > num_wires)
        return LookupReason::column_outside;
    if (l.q_look < num_selectors || l.q_tab < num_selectors) return LookupReason::marker_is_selector;
    if (l.tagged() && (l.tag_const0 < num_selectors || (uint64_t)l.tag_const0 + 1 >= num_constants)) return LookupReason::tag_columns;
    return LookupReason::ok;
}

// ---- the options of a gates-as-data proof ----------------------------------------------------------------------------------------------
// What the sibling entries sipp_plonk_prove_gates{,_lookup,_zk,_h} differ in, as the ONE value behind them (plonk.hip sipp_prove_gates;
// internal, not part of the ABI).  The defaults are every option off.
struct ProveOptions {
    const uint32_t* lookup = nullptr;           // the eight words of a lookup description; nullptr: the empty one
    const sipp_blinding* blind = nullptr;       // the seed and counter of a zero-knowledge proof; nullptr: none
    uint32_t hasher = SIPP_HASH_POSEIDON;
    // a hiding fp and no seed is refused at the options (SIPP_E_BADARG) unless this is set: the two entries older than blinding, which
    // take no seed, set it and keep the answer plonk_prove_impl has always given them (SIPP_E_UNSUPPORTED)
    bool missing_seed_left_to_prover = false;
};

// ---- the gate set ----------------------------------------------------------------------------------------------------------------------
enum class Circuit { ok, description, selector_group, past_program_words, program, operand };
// the STRUCTURE of a gate set handed over as data: every operand in range, every program inside program_words -- an index out of range
// would be a read outside the LDE buffers (the prover) or the opened values (the verifier)
inline Circuit circuit_walk(const sipp_plonk_circuit* c, const sipp_plonk_params* p) {
    if (!c || !p || c->num_wires < p->num_routed_wires || c->num_selectors == 0 || c->num_selectors > c->num_constants || c->num_gates == 0 ||
        !c->gates || (!c->programs && c->program_words))
        return Circuit::description;
    for (uint32_t g = 0; g < c->num_gates; g++) {
        const sipp_plonk_gate& ga = c->gates[g];
        if (ga.selector_index >= c->num_selectors || ga.group_lo > ga.row || ga.row >= ga.group_hi || ga.group_hi > c->num_gates)
            return Circuit::selector_group;
        size_t w = ga.prog_offset;
        for (uint32_t j = 0; j < ga.num_constraints; j++) {
            if (w >= c->program_words) return Circuit::past_program_words;
            const int64_t nm = c->programs[w++];
            if (nm < 0 || nm > 4096) return Circuit::program;
            for (int64_t m = 0; m < nm; m++) {
                if (w + 2 > c->program_words) return Circuit::past_program_words;
                const int64_t nf = c->programs[w + 1];
                w += 2;
                if (nf < 0 || nf > 64 || w + 2 * (size_t)nf > c->program_words) return Circuit::past_program_words;
                for (int64_t f = 0; f < nf; f++, w += 2) {
                    const int64_t kind = c->programs[w], idx = c->programs[w + 1];
                    if (kind < 0 || kind > 2 || idx < 0 || (kind == 0 && idx >= c->num_wires) || (kind == 1 && idx >= c->num_constants) ||
                        (kind == 2 && idx >= 4))
                        return Circuit::operand;
                }
            }
        }
    }
    return Circuit::ok;
}
// the PROVER's caps on a gate set that circuit_walk has passed (the verifier applies none of them to a circuit without lookups)
inline Circuit circuit_caps(const sipp_plonk_circuit& c) {
    if (!sizes_within_caps(c.num_wires, c.num_constants) || c.num_gates > 4096) return Circuit::description;
    for (uint32_t g = 0; g < c.num_gates; g++)
        if (c.gates[g].group_hi - c.gates[g].group_lo > 64 || c.gates[g].num_constraints > 4096) return Circuit::selector_group;
    return Circuit::ok;
}

}  // namespace plonk_desc
