// sipp_amd/csrc/circuit_data.hip -- plonky2's CircuitData for the outer proof behind HOST pointers: what the reference does at
// src/verifier_circuit.rs:225 (`builder.build::<C>()`: constants_sigmas committed once, the generators ordered once), :253 (`data.prove(pw)`)
// and :254 (`data.verify(proof)`), for a caller that holds no device memory of its own (the Rust shim; include/sipp_host.hpp's CircuitData).
// Nothing new is computed here: build = sipp_commit_batch_ex over the uploaded constants_sigmas; prove = upload of the wire table with its
// input cells (or a scatter of the input cells alone into a zeroed table), sipp_plonk_generate_witness[_levels]_blind, the path behind
// sipp_plonk_prove_gates* (sipp_prove_gates) with the data's lookup description, seed and number of the proof, and hasher; verify =
// sipp_plonk_verify_gates_h with the data's own cap / digest.
// Device memory of a circuit data is its own (hipMalloc at build: the arena of the ctx is the provers' scratch and empties after each proof).
#include "ctx.hpp"
#include "host_challenger.hpp"

#include <memory>

struct sipp_circuit_data {
    sipp_ctx* ctx = nullptr;
    uint32_t log_n = 0;
    sipp_plonk_params p{};
    sipp_fri_params fp{};
    sipp_plonk_circuit circ{};
    std::vector<sipp_plonk_gate> gates;
    std::vector<int64_t> programs;
    std::vector<sipp_plonk_generator> gens;
    bool has_sched = false;
    sipp_plonk_schedule sched{};
    std::vector<uint32_t> level_offsets, copy_offsets;
    std::vector<void*> dev;                 // everything hipMalloc'ed for this circuit
    uint64_t *d_cs = nullptr, *d_wires = nullptr;
    sipp_oracle cs_oracle{};
    std::vector<uint64_t> cap;
    uint64_t digest[4] = {0, 0, 0, 0};
    // the input map of sipp_circuit_set_input_map: cells then sources in one block of its own (replaced as a whole, so not in `dev`)
    uint64_t* d_map = nullptr;
    size_t map_n = 0, map_words = 0, map_extra = 0;
    bool has_map = false;
    // the lookup description of sipp_circuit_set_lookup (all zero: none), as the eight words the C calls take and as their one reading,
    // and the sorted index of its table, a block of its own like the map
    uint32_t lookup[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    plonk_desc::Lookup lk{};
    uint64_t* d_index = nullptr;
    uint32_t n_index = 0;
    // zero knowledge (a hiding fp): the seed of sipp_circuit_set_blinding and the number of the next proof under it
    sipp_blinding blind{};
    bool has_blind = false;
    // the tree hasher of sipp_circuit_build_h: of the constants_sigmas commitment below and of every proof and verification
    uint32_t hasher = SIPP_HASH_POSEIDON;
    ~sipp_circuit_data() {
        if (ctx) (void)hipSetDevice(ctx->device);
        for (void* q : dev) (void)hipFree(q);
        if (d_map) (void)hipFree(d_map);
        if (d_index) (void)hipFree(d_index);
    }
};

namespace {
template <typename T>
int dev_alloc(sipp_circuit_data* cd, size_t count, T** out) {
    void* q = nullptr;
    if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return sipp_fail(cd->ctx, SIPP_E_NOMEM, "circuit data: hipMalloc failed");
    cd->dev.push_back(q);
    *out = reinterpret_cast<T*>(q);
    return SIPP_OK;
}
template <typename T>
int dev_upload(sipp_circuit_data* cd, const T* host, size_t count, T** out) {
    SIPP_TRY(dev_alloc(cd, count, out));
    if (count) SIPP_CHECK_HIP(cd->ctx, hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice));
    return SIPP_OK;
}
// A block the data owns by itself (the input map, the lookup index) takes new contents: the new block is allocated and filled first, and
// only then does the old one go -- a refusal or a failed upload leaves the previous block, and what the caller keeps beside it, in
// force.  No kernel reads the old block any more: a proof ends on the host.  `parts`: host arrays laid back to back, `count` words each;
// `who` opens the messages
int replace_block(sipp_circuit_data* cd, uint64_t** block, std::initializer_list<const uint64_t*> parts, size_t count, const std::string& who) {
    sipp_ctx* ctx = cd->ctx;
    void* q = nullptr;
    if (hipMalloc(&q, (count ? parts.size() * count : 1) * 8) != hipSuccess) return sipp_fail(ctx, SIPP_E_NOMEM, (who + ": hipMalloc failed").c_str());
    uint64_t* d_new = reinterpret_cast<uint64_t*>(q);
    size_t at = 0;
    for (const uint64_t* part : parts) {
        if (count && hipMemcpy(d_new + at, part, count * 8, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(q);
            return sipp_fail(ctx, SIPP_E_HIP, (who + ": upload failed").c_str());
        }
        at += count;
    }
    if (*block) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(*block);
    }
    *block = d_new;
    return SIPP_OK;
}
uint32_t zs_columns(const sipp_plonk_params* p) { return p->num_challenges * ((p->num_routed_wires + p->max_degree - 1) / p->max_degree); }
}  // namespace

extern "C" size_t sipp_circuit_workspace_bytes(uint32_t log_n, const sipp_plonk_params* p, const sipp_fri_params* fp, const sipp_plonk_circuit* c) {
    if (!p || !fp || !c || log_n > 26 || !p->max_degree) return 0;
    // every oracle the prover commits inside the call (wires, Z / partial products, quotient chunks): coefficients + LDE, and the
    // quotient's own working set; the constants_sigmas oracle lives outside the arena
    const size_t n = (size_t)1 << log_n, cols = (size_t)c->num_wires + zs_columns(p) + (size_t)p->num_challenges * p->max_degree;
    // (a hiding fp: four salt columns behind the LDE of each of the three)
    const size_t salt = fp->hiding ? (size_t)3 * SIPP_SALT_SIZE << fp->rate_bits : 0;
    return 8 * n * (((size_t)1 + ((size_t)1 << fp->rate_bits)) * (cols + c->num_constants + p->num_routed_wires) + salt + 64) + ((size_t)4 << 30);
}

extern "C" void sipp_circuit_destroy(sipp_circuit_data* cd) {
    if (!cd) return;
    if (cd->ctx && cd->ctx->stream) {
        (void)hipSetDevice(cd->ctx->device);
        (void)hipStreamSynchronize(cd->ctx->stream);
        sipp_witness_graph_release(cd->ctx);          // a captured schedule names this circuit's buffers
    }
    delete cd;
}

extern "C" int sipp_circuit_build(sipp_ctx* ctx, uint32_t log_n, const sipp_plonk_params* p, const sipp_fri_params* fp, const sipp_plonk_circuit* c,
                                  const uint64_t* constants_sigmas, const sipp_plonk_generator* gens, size_t n_gens,
                                  const sipp_plonk_schedule_host* sched, const uint64_t* circuit_digest, sipp_circuit_data** out) {
    return sipp_circuit_build_h(ctx, log_n, p, fp, c, constants_sigmas, gens, n_gens, sched, circuit_digest, SIPP_HASH_POSEIDON, out);
}

extern "C" int sipp_circuit_build_h(sipp_ctx* ctx, uint32_t log_n, const sipp_plonk_params* p, const sipp_fri_params* fp, const sipp_plonk_circuit* c,
                                    const uint64_t* constants_sigmas, const sipp_plonk_generator* gens, size_t n_gens,
                                    const sipp_plonk_schedule_host* sched, const uint64_t* circuit_digest, uint32_t hasher,
                                    sipp_circuit_data** out) {
    if (out) *out = nullptr;
    if (!ctx) return SIPP_E_BADARG;
    SIPP_TRY(sipp_hasher_check(ctx, hasher));
    if (!out || !p || !fp || !c || !constants_sigmas || (!gens && n_gens) || log_n < 1 || log_n > 24 || !c->gates || (!c->programs && c->program_words) ||
        !c->num_gates || c->num_wires < p->num_routed_wires)
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit build: null argument, log_n outside 1 .. 24 or an empty circuit");
    if (sched && sched->n_levels &&
        (!sched->rows || !sched->level_offsets || !sched->copy_offsets ||
         (sched->copy_offsets[sched->n_levels] && (!sched->copy_src || !sched->copy_dst)) || sched->n_levels > (1u << 20)))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit build: incomplete schedule");
    // sipp_plonk_generate_witness_levels' ceiling, refused here and not at the first proof (the row-local call has none)
    if (sched && sched->n_levels && n_gens > 32)
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit build: more than 32 generators with a level schedule");
    SIPP_TRY(sipp_plonk_circuit_check(ctx, c, p));          // a malformed gate set is refused here, not at the first proof
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // owned from here to `*out`: every return in between, the SIPP_TRY / SIPP_CHECK_HIP ones included, releases the object and its device memory
    std::unique_ptr<sipp_circuit_data> owner;
    sipp_circuit_data* cd = nullptr;
    try {
        owner.reset(cd = new sipp_circuit_data());
        cd->ctx = ctx; cd->log_n = log_n; cd->p = *p; cd->fp = *fp; cd->hasher = hasher;
        cd->gates.assign(c->gates, c->gates + c->num_gates);
        cd->programs.assign(c->programs, c->programs + c->program_words);
        cd->gens.assign(gens, gens + n_gens);
        if (sched && sched->n_levels) {
            cd->level_offsets.assign(sched->level_offsets, sched->level_offsets + sched->n_levels + 1);
            cd->copy_offsets.assign(sched->copy_offsets, sched->copy_offsets + sched->n_levels + 1);
        }
    } catch (const std::bad_alloc&) {
        return sipp_fail(ctx, SIPP_E_NOMEM, "circuit build: host allocation failed");
    }
    cd->circ = *c;
    cd->circ.gates = cd->gates.data();
    cd->circ.programs = cd->programs.data();
    const size_t n = (size_t)1 << log_n, ncols = (size_t)c->num_constants + p->num_routed_wires, m = n << fp->rate_bits;
    if (sched && sched->n_levels) {
        const uint32_t L = sched->n_levels;
        for (uint32_t l = 0; l < L; l++)
            if (sched->level_offsets[l] > sched->level_offsets[l + 1] || sched->copy_offsets[l] > sched->copy_offsets[l + 1])
                return sipp_fail(ctx, SIPP_E_BADARG, "circuit build: schedule offsets must not decrease");
        if (sched->level_offsets[L] > n) return sipp_fail(ctx, SIPP_E_BADARG, "circuit build: more scheduled rows than the table has");
        uint32_t* d_rows = nullptr;
        uint64_t *d_src = nullptr, *d_dst = nullptr;
        SIPP_TRY(dev_upload(cd, sched->rows, sched->level_offsets[L], &d_rows));
        SIPP_TRY(dev_upload(cd, sched->copy_src, sched->copy_offsets[L], &d_src));
        SIPP_TRY(dev_upload(cd, sched->copy_dst, sched->copy_offsets[L], &d_dst));
        cd->has_sched = true;
        cd->sched.n_levels = L; cd->sched.d_rows = d_rows; cd->sched.d_copy_src = d_src; cd->sched.d_copy_dst = d_dst;
        cd->sched.level_offsets = cd->level_offsets.data(); cd->sched.copy_offsets = cd->copy_offsets.data();
    }
    uint64_t *d_coeffs = nullptr, *d_lde = nullptr, *d_tree = nullptr;
    SIPP_TRY(dev_upload(cd, constants_sigmas, ncols * n, &cd->d_cs));
    SIPP_TRY(dev_alloc(cd, (size_t)c->num_wires * n, &cd->d_wires));
    SIPP_TRY(dev_alloc(cd, ncols * n, &d_coeffs));
    SIPP_TRY(dev_alloc(cd, ncols * m, &d_lde));
    SIPP_TRY(dev_alloc(cd, 2 * m * 4, &d_tree));
    const uint32_t ch = fp->cap_height < log_n + fp->rate_bits ? fp->cap_height : log_n + fp->rate_bits;
    cd->cap.assign(((size_t)4) << ch, 0);
    SIPP_TRY(sipp_commit_batch_h(ctx, cd->d_cs, 0, d_coeffs, d_lde, d_tree, ncols, log_n, fp->rate_bits, fp->cap_height, nullptr, 0, hasher, cd->cap.data()));
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    cd->cs_oracle.d_coeffs = d_coeffs; cd->cs_oracle.d_lde = d_lde; cd->cs_oracle.d_tree = d_tree;
    cd->cs_oracle.n_polys = (uint32_t)ncols; cd->cs_oracle.n_salt = 0;
    if (circuit_digest) {
        for (int q = 0; q < 4; q++) cd->digest[q] = circuit_digest[q];
    } else {
        std::vector<uint64_t> w(cd->cap);
        for (uint64_t v : {(uint64_t)log_n, (uint64_t)c->num_wires, (uint64_t)p->num_routed_wires, (uint64_t)c->num_constants, (uint64_t)c->num_selectors,
                           (uint64_t)c->num_gates})
            w.push_back(v);
        host::Challenger::hash_no_pad(w.data(), w.size(), cd->digest);
    }
    if (sipp_plonk_gates_proof_size(log_n, p, fp, &cd->circ, 0) == 0) return sipp_fail(ctx, SIPP_E_BADARG, "circuit build: parameters or gate set refused");
    *out = owner.release();
    return SIPP_OK;
}

extern "C" int sipp_circuit_verifier_data(const sipp_circuit_data* cd, uint64_t* cap_out, uint64_t* digest_out) {
    if (!cd || !cap_out || !digest_out) return SIPP_E_BADARG;
    std::copy(cd->cap.begin(), cd->cap.end(), cap_out);
    for (int q = 0; q < 4; q++) digest_out[q] = cd->digest[q];
    return SIPP_OK;
}

extern "C" size_t sipp_circuit_proof_size(const sipp_circuit_data* cd, uint32_t n_public_inputs) {
    return cd ? sipp_gates_proof_words(cd->log_n, &cd->p, &cd->fp, &cd->circ, n_public_inputs, cd->lookup, cd->fp.hiding != 0) : 0;
}

namespace {
// The blinding of ONE prove call: the data's seed with the current counter, which moves on at once -- so a call that is refused
// further down has used its number up as well.  `use` is nullptr for a data that is not hiding.
struct BlindTicket {
    sipp_blinding b{};
    const uint64_t* use = nullptr;      // its five words, as the C calls take them
    explicit BlindTicket(sipp_circuit_data* cd) {
        if (!cd->has_blind) return;
        b = cd->blind;
        use = b.seed;
        cd->blind.counter++;
    }
};
// a hiding circuit data proves only with a seed
int blind_ready(sipp_circuit_data* cd) {
    return cd->fp.hiding && !cd->has_blind ? sipp_fail(cd->ctx, SIPP_E_BADARG, "circuit prove: hiding FRI parameters and no seed (sipp_circuit_set_blinding)")
                                           : SIPP_OK;
}

// what both prove calls do once the device wire table holds the input cells
int prove_uploaded(sipp_circuit_data* cd, const uint64_t* blind, const uint64_t* public_inputs, uint32_t n_public_inputs, uint64_t* proof_out,
                   size_t proof_cap, size_t* proof_len) {
    sipp_ctx* ctx = cd->ctx;
    uint64_t pih[4];
    host::Challenger::hash_no_pad(public_inputs, n_public_inputs, pih);
    if (cd->has_sched)
        SIPP_TRY(sipp_plonk_generate_witness_levels_blind(ctx, cd->d_wires, cd->d_cs, cd->log_n, cd->circ.num_wires, cd->circ.num_constants,
                                                          cd->gens.data(), cd->gens.size(), pih, &cd->sched, blind));
    else
        SIPP_TRY(sipp_plonk_generate_witness_blind(ctx, cd->d_wires, cd->d_cs, cd->log_n, cd->circ.num_wires, cd->circ.num_constants,
                                                   cd->gens.data(), cd->gens.size(), pih, blind));
    // the multiplicities behind witness generation: the looking wires are the generators' outputs (or the caller's cells)
    if (!cd->lk.empty()) SIPP_TRY(sipp_lookup_multiplicities_indexed(ctx, cd->d_wires, cd->d_cs, cd->log_n, cd->lk, cd->d_index, cd->n_index));
    const BlindArg arg(blind);      // the one path behind the sibling entries serves every kind of proof
    const plonk_desc::ProveOptions o{cd->lookup, arg.p, cd->hasher};
    return sipp_prove_gates(ctx, cd->d_wires, cd->d_cs, nullptr, nullptr, &cd->cs_oracle, cd->log_n, &cd->p, &cd->fp, &cd->circ, cd->digest, public_inputs,
                            n_public_inputs, o, proof_out, proof_cap, proof_len);
}

// The input cells of a proof: pair k puts its value at cells[k], one lane per pair, grid-stride.  MAPPED: the value is
// staged[sources[k]] (sipp_circuit_prove_words: the staged words through the data's input map; every source is below the staged length,
// sipp_circuit_set_input_map refuses a map where one is not), else staged[k] (sipp_circuit_prove_inputs).  Pairs that name one cell race;
// whichever store lands, the check pass sees every pair whose value the table does not hold.
template <bool MAPPED>
__global__ void __launch_bounds__(256) circuit_scatter_kernel(uint64_t* wires, const uint64_t* cells, const uint64_t* sources, const uint64_t* staged,
                                                              size_t count) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) wires[cells[k]] = staged[MAPPED ? sources[k] : k];
}
template <bool MAPPED>
__global__ void __launch_bounds__(256) circuit_check_kernel(const uint64_t* wires, const uint64_t* cells, const uint64_t* sources, const uint64_t* staged,
                                                            size_t count, unsigned int* conflict) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) bad |= wires[cells[k]] != staged[MAPPED ? sources[k] : k];
    if (bad) atomicOr(conflict, 1u);
}

// zero the wire table, scatter the `count` pairs, check them, wait for the flag and refuse, with the caller's words, one cell that took
// two different values.  Device pointers (every cell below the table's size: the callers' host checks); d_sources == nullptr: pair k
// takes d_staged[k].  The wait has ended every kernel that reads the caller's staging, which may go back to the arena before witness generation.
int stage_inputs(sipp_circuit_data* cd, const uint64_t* d_cells, const uint64_t* d_sources, const uint64_t* d_staged, size_t count,
                 unsigned int* d_conflict, const char* refusal) {
    sipp_ctx* ctx = cd->ctx;
    SIPP_CHECK_HIP(ctx, hipMemsetAsync(cd->d_wires, 0, ((size_t)cd->circ.num_wires << cd->log_n) * 8, ctx->stream));
    if (!count) return SIPP_OK;
    SIPP_CHECK_HIP(ctx, hipMemsetAsync(d_conflict, 0, 8, ctx->stream));
    const size_t want = (count + 255) / 256;
    const dim3 grid((unsigned)(want < 4096 ? want : 4096));
    hipLaunchKernelGGL(d_sources ? circuit_scatter_kernel<true> : circuit_scatter_kernel<false>, grid, dim3(256), 0, ctx->stream, cd->d_wires, d_cells,
                       d_sources, d_staged, count);
    hipLaunchKernelGGL(d_sources ? circuit_check_kernel<true> : circuit_check_kernel<false>, grid, dim3(256), 0, ctx->stream, cd->d_wires, d_cells,
                       d_sources, d_staged, count, d_conflict);
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    unsigned int flag = 0;
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(&flag, d_conflict, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return flag ? sipp_fail(ctx, SIPP_E_BADARG, refusal) : SIPP_OK;
}
}  // namespace

extern "C" int sipp_circuit_set_input_map(sipp_circuit_data* cd, const uint64_t* cells, const uint64_t* sources, size_t n, size_t n_words,
                                          size_t n_extra) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if ((n && (!cells || !sources)) || n > ((size_t)1 << 40) || n_words > ((size_t)1 << 40) || n_extra > ((size_t)1 << 40))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit input map: null argument or a count out of range");
    const size_t total = (size_t)cd->circ.num_wires << cd->log_n, staged = n_words + n_extra;
    for (size_t k = 0; k < n; k++) {
        if (cells[k] >= total) return sipp_fail(ctx, SIPP_E_BADARG, "circuit input map: a cell outside the wire table");
        if (sources[k] >= staged) return sipp_fail(ctx, SIPP_E_BADARG, "circuit input map: a source outside words || extra");
    }
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    SIPP_TRY(replace_block(cd, &cd->d_map, {cells, sources}, n, "circuit input map"));
    cd->map_n = n; cd->map_words = n_words; cd->map_extra = n_extra; cd->has_map = true;
    return SIPP_OK;
}

extern "C" int sipp_circuit_set_blinding(sipp_circuit_data* cd, const uint64_t seed[4]) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if (!seed) return sipp_fail(ctx, SIPP_E_BADARG, "circuit blinding: no seed");
    if (!cd->fp.hiding) return sipp_fail(ctx, SIPP_E_BADARG, "circuit blinding: the circuit data was built without hiding FRI parameters");
    const sipp_blinding b{{seed[0], seed[1], seed[2], seed[3]}, 0};
    SIPP_TRY(sipp_blind_check(ctx, &b));
    cd->blind = b;
    cd->has_blind = true;
    return SIPP_OK;
}

extern "C" int sipp_circuit_set_lookup(sipp_circuit_data* cd, const uint32_t* lookup) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    plonk_desc::Lookup l;
    SIPP_TRY(sipp_lookup_check(ctx, lookup, cd->circ.num_wires, cd->circ.num_constants, cd->circ.num_selectors, &l));
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> index;
    if (!l.empty()) {
        if (sipp_gates_proof_words(cd->log_n, &cd->p, &cd->fp, &cd->circ, 0, lookup, false) == 0)
            return sipp_fail(ctx, SIPP_E_BADARG, "circuit lookup: the description does not fit the parameters");
        SIPP_TRY(sipp_lookup_index_host(ctx, cd->d_cs, cd->log_n, l, &index));
        SIPP_TRY(replace_block(cd, &cd->d_index, {index.data()}, index.size(), "circuit lookup"));
    } else if (cd->d_index) {      // back to no lookups: the index goes, behind every refusal like a replaced one
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(cd->d_index);
        cd->d_index = nullptr;
    }
    cd->n_index = (uint32_t)(index.size() / 4);
    cd->lk = l.empty() ? plonk_desc::Lookup{} : l;
    for (int q = 0; q < 8; q++) cd->lookup[q] = l.empty() ? 0 : lookup[q];
    return SIPP_OK;
}

extern "C" int sipp_circuit_prove(sipp_circuit_data* cd, const uint64_t* wires, const uint64_t* public_inputs, uint32_t n_public_inputs,
                                  uint64_t* proof_out, size_t proof_cap, size_t* proof_len) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if (!wires || !proof_out || !proof_len || (n_public_inputs && !public_inputs) || n_public_inputs > (1u << 24))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove: null argument");
    SIPP_TRY(blind_ready(cd));
    const BlindTicket ticket(cd);
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << cd->log_n;
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(cd->d_wires, wires, (size_t)cd->circ.num_wires * n * 8, hipMemcpyHostToDevice, ctx->stream));
    return prove_uploaded(cd, ticket.use, public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
}

extern "C" int sipp_circuit_prove_inputs(sipp_circuit_data* cd, const uint64_t* cells, const uint64_t* values, size_t n_inputs,
                                         const uint64_t* public_inputs, uint32_t n_public_inputs, uint64_t* proof_out, size_t proof_cap,
                                         size_t* proof_len) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if ((n_inputs && (!cells || !values)) || !proof_out || !proof_len || (n_public_inputs && !public_inputs) || n_public_inputs > (1u << 24))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove inputs: null argument");
    SIPP_TRY(blind_ready(cd));
    const BlindTicket ticket(cd);
    const size_t total = (size_t)cd->circ.num_wires << cd->log_n;
    if (n_inputs > ((size_t)1 << 40)) return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove inputs: too many pairs");
    for (size_t k = 0; k < n_inputs; k++)
        if (cells[k] >= total) return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove inputs: a cell outside the wire table");
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    {
        // the staging goes back before witness generation: the wait for the flag has then ended every kernel that reads it
        ArenaScope scope(ctx);
        uint64_t* d_pairs = arena_alloc_t<uint64_t>(ctx, 2 * n_inputs + 1);          // cells, values, the flag's word
        if (!d_pairs) return SIPP_E_NOMEM;
        uint64_t *d_cells = d_pairs, *d_values = d_pairs + n_inputs;
        if (n_inputs) {
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_cells, cells, n_inputs * 8, hipMemcpyHostToDevice, ctx->stream));
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_values, values, n_inputs * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        SIPP_TRY(stage_inputs(cd, d_cells, nullptr, d_values, n_inputs, reinterpret_cast<unsigned int*>(d_pairs + 2 * n_inputs),
                              "circuit prove inputs: one cell given two different values"));
    }
    return prove_uploaded(cd, ticket.use, public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
}

extern "C" int sipp_circuit_prove_words(sipp_circuit_data* cd, const uint64_t* words, size_t n_words, const uint64_t* extra, size_t n_extra,
                                        const uint64_t* public_inputs, uint32_t n_public_inputs, uint64_t* proof_out, size_t proof_cap,
                                        size_t* proof_len) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if ((n_words && !words) || (n_extra && !extra) || !proof_out || !proof_len || (n_public_inputs && !public_inputs) || n_public_inputs > (1u << 24))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: null argument");
    SIPP_TRY(blind_ready(cd));
    const BlindTicket ticket(cd);
    if (!cd->has_map) return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: no input map set (sipp_circuit_set_input_map)");
    if (n_words != cd->map_words || n_extra != cd->map_extra)
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: n_words / n_extra differ from the input map's");
    const size_t n = cd->map_n;
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    {
        // as in sipp_circuit_prove_inputs: the staging goes back before witness generation, behind the wait for the flag
        ArenaScope scope(ctx);
        uint64_t* d_staged = arena_alloc_t<uint64_t>(ctx, n_words + n_extra + 1);        // words, extra, the flag's word
        if (!d_staged) return SIPP_E_NOMEM;
        if (n && n_words) SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_staged, words, n_words * 8, hipMemcpyHostToDevice, ctx->stream));
        if (n && n_extra) SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_staged + n_words, extra, n_extra * 8, hipMemcpyHostToDevice, ctx->stream));
        SIPP_TRY(stage_inputs(cd, cd->d_map, cd->d_map + n, d_staged, n, reinterpret_cast<unsigned int*>(d_staged + n_words + n_extra),
                              "circuit prove words: one cell mapped to two different values"));
    }
    return prove_uploaded(cd, ticket.use, public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
}

extern "C" int sipp_circuit_verify(const sipp_circuit_data* cd, const uint64_t* proof, size_t len, int* reason) {
    if (!cd) return SIPP_E_BADARG;
    return sipp_plonk_verify_gates_h(proof, len, cd->cap.data(), &cd->p, &cd->fp, &cd->circ, cd->digest, cd->lookup, cd->hasher, reason);
}
