// sipp_amd/csrc/circuit_data.hip -- plonky2's CircuitData for the outer proof behind HOST pointers: what the reference does at
// src/verifier_circuit.rs:225 (`builder.build::<C>()`: constants_sigmas committed once, the generators ordered once), :253 (`data.prove(pw)`)
// and :254 (`data.verify(proof)`), for a caller that holds no device memory of its own (the Rust shim; include/sipp_host.hpp's CircuitData).
// Nothing new is computed here: build = sipp_commit_batch_ex over the uploaded constants_sigmas; prove = upload of the wire table with its
// input cells (or a scatter of the input cells alone into a zeroed table), sipp_plonk_generate_witness[_levels], sipp_plonk_prove_gates; verify = sipp_plonk_verify_gates with the data's own cap / digest.
// Device memory of a circuit data is its own (hipMalloc at build: the arena of the ctx is the provers' scratch and empties after each proof).
#include "ctx.hpp"
#include "host_challenger.hpp"

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
    // the lookup description of sipp_circuit_set_lookup (all zero: none) and the sorted index of its table, a block of its own like the map
    uint32_t lookup[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t* d_index = nullptr;
    uint32_t n_index = 0;
    bool has_lookup() const { return lookup[2] != 0; }
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
uint32_t zs_columns(const sipp_plonk_params* p) { return p->num_challenges * ((p->num_routed_wires + p->max_degree - 1) / p->max_degree); }
}  // namespace

extern "C" size_t sipp_circuit_workspace_bytes(uint32_t log_n, const sipp_plonk_params* p, const sipp_fri_params* fp, const sipp_plonk_circuit* c) {
    if (!p || !fp || !c || log_n > 26 || !p->max_degree) return 0;
    // every oracle the prover commits inside the call (wires, Z / partial products, quotient chunks): coefficients + LDE, and the
    // quotient's own working set; the constants_sigmas oracle lives outside the arena
    const size_t n = (size_t)1 << log_n, cols = (size_t)c->num_wires + zs_columns(p) + (size_t)p->num_challenges * p->max_degree;
    return 8 * n * (((size_t)1 + ((size_t)1 << fp->rate_bits)) * (cols + c->num_constants + p->num_routed_wires) + 64) + ((size_t)4 << 30);
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
    if (out) *out = nullptr;
    if (!ctx) return SIPP_E_BADARG;
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
    sipp_circuit_data* cd = nullptr;
    try {
        cd = new sipp_circuit_data();
        cd->ctx = ctx; cd->log_n = log_n; cd->p = *p; cd->fp = *fp;
        cd->gates.assign(c->gates, c->gates + c->num_gates);
        cd->programs.assign(c->programs, c->programs + c->program_words);
        cd->gens.assign(gens, gens + n_gens);
        if (sched && sched->n_levels) {
            cd->level_offsets.assign(sched->level_offsets, sched->level_offsets + sched->n_levels + 1);
            cd->copy_offsets.assign(sched->copy_offsets, sched->copy_offsets + sched->n_levels + 1);
        }
    } catch (const std::bad_alloc&) {
        delete cd;
        return sipp_fail(ctx, SIPP_E_NOMEM, "circuit build: host allocation failed");
    }
    cd->circ = *c;
    cd->circ.gates = cd->gates.data();
    cd->circ.programs = cd->programs.data();
    auto bail = [&](int rc) {
        delete cd;
        return rc;
    };
    const size_t n = (size_t)1 << log_n, ncols = (size_t)c->num_constants + p->num_routed_wires, m = n << fp->rate_bits;
    int rc;
    if (sched && sched->n_levels) {
        const uint32_t L = sched->n_levels;
        for (uint32_t l = 0; l < L; l++)
            if (sched->level_offsets[l] > sched->level_offsets[l + 1] || sched->copy_offsets[l] > sched->copy_offsets[l + 1])
                return bail(sipp_fail(ctx, SIPP_E_BADARG, "circuit build: schedule offsets must not decrease"));
        if (sched->level_offsets[L] > n) return bail(sipp_fail(ctx, SIPP_E_BADARG, "circuit build: more scheduled rows than the table has"));
        uint32_t* d_rows = nullptr;
        uint64_t *d_src = nullptr, *d_dst = nullptr;
        if ((rc = dev_upload(cd, sched->rows, sched->level_offsets[L], &d_rows)) != SIPP_OK) return bail(rc);
        if ((rc = dev_upload(cd, sched->copy_src, sched->copy_offsets[L], &d_src)) != SIPP_OK) return bail(rc);
        if ((rc = dev_upload(cd, sched->copy_dst, sched->copy_offsets[L], &d_dst)) != SIPP_OK) return bail(rc);
        cd->has_sched = true;
        cd->sched.n_levels = L; cd->sched.d_rows = d_rows; cd->sched.d_copy_src = d_src; cd->sched.d_copy_dst = d_dst;
        cd->sched.level_offsets = cd->level_offsets.data(); cd->sched.copy_offsets = cd->copy_offsets.data();
    }
    uint64_t *d_coeffs = nullptr, *d_lde = nullptr, *d_tree = nullptr;
    if ((rc = dev_upload(cd, constants_sigmas, ncols * n, &cd->d_cs)) != SIPP_OK) return bail(rc);
    if ((rc = dev_alloc(cd, (size_t)c->num_wires * n, &cd->d_wires)) != SIPP_OK) return bail(rc);
    if ((rc = dev_alloc(cd, ncols * n, &d_coeffs)) != SIPP_OK) return bail(rc);
    if ((rc = dev_alloc(cd, ncols * m, &d_lde)) != SIPP_OK) return bail(rc);
    if ((rc = dev_alloc(cd, 2 * m * 4, &d_tree)) != SIPP_OK) return bail(rc);
    const uint32_t ch = fp->cap_height < log_n + fp->rate_bits ? fp->cap_height : log_n + fp->rate_bits;
    cd->cap.assign(((size_t)4) << ch, 0);
    rc = sipp_commit_batch_ex(ctx, cd->d_cs, 0, d_coeffs, d_lde, d_tree, ncols, log_n, fp->rate_bits, fp->cap_height, nullptr, 0, cd->cap.data());
    if (rc != SIPP_OK) return bail(rc);
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
    if (sipp_plonk_gates_proof_size(log_n, p, fp, &cd->circ, 0) == 0) return bail(sipp_fail(ctx, SIPP_E_BADARG, "circuit build: parameters or gate set refused"));
    *out = cd;
    return SIPP_OK;
}

extern "C" int sipp_circuit_verifier_data(const sipp_circuit_data* cd, uint64_t* cap_out, uint64_t* digest_out) {
    if (!cd || !cap_out || !digest_out) return SIPP_E_BADARG;
    std::copy(cd->cap.begin(), cd->cap.end(), cap_out);
    for (int q = 0; q < 4; q++) digest_out[q] = cd->digest[q];
    return SIPP_OK;
}

extern "C" size_t sipp_circuit_proof_size(const sipp_circuit_data* cd, uint32_t n_public_inputs) {
    return cd ? sipp_plonk_gates_lookup_proof_size(cd->log_n, &cd->p, &cd->fp, &cd->circ, n_public_inputs, cd->lookup) : 0;
}

namespace {
// what both prove calls do once the device wire table holds the input cells
int prove_uploaded(sipp_circuit_data* cd, const uint64_t* public_inputs, uint32_t n_public_inputs, uint64_t* proof_out, size_t proof_cap,
                   size_t* proof_len) {
    sipp_ctx* ctx = cd->ctx;
    uint64_t pih[4];
    host::Challenger::hash_no_pad(public_inputs, n_public_inputs, pih);
    if (cd->has_sched)
        SIPP_TRY(sipp_plonk_generate_witness_levels(ctx, cd->d_wires, cd->d_cs, cd->log_n, cd->circ.num_wires, cd->circ.num_constants, cd->gens.data(),
                                                    cd->gens.size(), pih, &cd->sched));
    else
        SIPP_TRY(sipp_plonk_generate_witness(ctx, cd->d_wires, cd->d_cs, cd->log_n, cd->circ.num_wires, cd->circ.num_constants, cd->gens.data(),
                                             cd->gens.size(), pih));
    if (!cd->has_lookup())
        return sipp_plonk_prove_gates(ctx, cd->d_wires, cd->d_cs, nullptr, nullptr, &cd->cs_oracle, cd->log_n, &cd->p, &cd->fp, &cd->circ, cd->digest,
                                      public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
    // the multiplicities behind witness generation: the looking wires are the generators' outputs (or the caller's cells)
    SIPP_TRY(sipp_lookup_multiplicities_indexed(ctx, cd->d_wires, cd->d_cs, cd->log_n, cd->lookup, cd->d_index, cd->n_index));
    return sipp_plonk_prove_gates_lookup(ctx, cd->d_wires, cd->d_cs, nullptr, nullptr, &cd->cs_oracle, cd->log_n, &cd->p, &cd->fp, &cd->circ,
                                         cd->digest, public_inputs, n_public_inputs, cd->lookup, proof_out, proof_cap, proof_len);
}

// the input cells of sipp_circuit_prove_inputs: one lane per pair, grid-stride.  Pairs that name one cell race; whichever store lands,
// the check pass below sees every pair whose value the table does not hold.
__global__ void __launch_bounds__(256) circuit_scatter_inputs_kernel(uint64_t* wires, const uint64_t* cells, const uint64_t* values, size_t count) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) wires[cells[k]] = values[k];
}
__global__ void __launch_bounds__(256) circuit_check_inputs_kernel(const uint64_t* wires, const uint64_t* cells, const uint64_t* values, size_t count,
                                                                   unsigned int* conflict) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) bad |= wires[cells[k]] != values[k];
    if (bad) atomicOr(conflict, 1u);
}
// the same two passes for sipp_circuit_prove_words: pair k takes its value from the staged words through the data's input map.  Every
// cell is below the table's size and every source below the staged length: sipp_circuit_set_input_map refuses a map where one is not.
__global__ void __launch_bounds__(256) circuit_scatter_words_kernel(uint64_t* wires, const uint64_t* cells, const uint64_t* sources,
                                                                    const uint64_t* staged, size_t count) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) wires[cells[k]] = staged[sources[k]];
}
__global__ void __launch_bounds__(256) circuit_check_words_kernel(const uint64_t* wires, const uint64_t* cells, const uint64_t* sources,
                                                                  const uint64_t* staged, size_t count, unsigned int* conflict) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += step) bad |= wires[cells[k]] != staged[sources[k]];
    if (bad) atomicOr(conflict, 1u);
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
    void* q = nullptr;
    if (hipMalloc(&q, (n ? 2 * n : 1) * 8) != hipSuccess) return sipp_fail(ctx, SIPP_E_NOMEM, "circuit input map: hipMalloc failed");
    uint64_t* d_new = reinterpret_cast<uint64_t*>(q);
    if (n && (hipMemcpy(d_new, cells, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(d_new + n, sources, n * 8, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipFree(q);
        return sipp_fail(ctx, SIPP_E_HIP, "circuit input map: upload failed");
    }
    // the old map goes only now: every refusal above has left it in force.  No kernel reads it any more: a proof ends on the host
    if (cd->d_map) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(cd->d_map);
    }
    cd->d_map = d_new; cd->map_n = n; cd->map_words = n_words; cd->map_extra = n_extra; cd->has_map = true;
    return SIPP_OK;
}

extern "C" int sipp_circuit_set_lookup(sipp_circuit_data* cd, const uint32_t* lookup) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    SIPP_TRY(sipp_lookup_check(ctx, lookup, cd->circ.num_wires, cd->circ.num_constants, cd->circ.num_selectors));
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const bool empty = lookup[2] == 0 && lookup[6] == 0;
    uint64_t* d_new = nullptr;
    std::vector<uint64_t> index;
    if (!empty) {
        if (sipp_plonk_gates_lookup_proof_size(cd->log_n, &cd->p, &cd->fp, &cd->circ, 0, lookup) == 0)
            return sipp_fail(ctx, SIPP_E_BADARG, "circuit lookup: the description does not fit the parameters");
        SIPP_TRY(sipp_lookup_index_host(ctx, cd->d_cs, cd->log_n, lookup, &index));
        void* q = nullptr;
        if (hipMalloc(&q, (index.empty() ? 1 : index.size()) * 8) != hipSuccess) return sipp_fail(ctx, SIPP_E_NOMEM, "circuit lookup: hipMalloc failed");
        d_new = reinterpret_cast<uint64_t*>(q);
        if (!index.empty() && hipMemcpy(d_new, index.data(), index.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(q);
            return sipp_fail(ctx, SIPP_E_HIP, "circuit lookup: upload failed");
        }
    }
    // the old index goes only now: every refusal above has left the description before in force.  No kernel reads it: a proof ends on the host
    if (cd->d_index) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(cd->d_index);
    }
    cd->d_index = d_new; cd->n_index = (uint32_t)(index.size() / 4);
    for (int q = 0; q < 8; q++) cd->lookup[q] = empty ? 0 : lookup[q];
    return SIPP_OK;
}

extern "C" int sipp_circuit_prove(sipp_circuit_data* cd, const uint64_t* wires, const uint64_t* public_inputs, uint32_t n_public_inputs,
                                  uint64_t* proof_out, size_t proof_cap, size_t* proof_len) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if (!wires || !proof_out || !proof_len || (n_public_inputs && !public_inputs) || n_public_inputs > (1u << 24))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove: null argument");
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << cd->log_n;
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(cd->d_wires, wires, (size_t)cd->circ.num_wires * n * 8, hipMemcpyHostToDevice, ctx->stream));
    return prove_uploaded(cd, public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
}

extern "C" int sipp_circuit_prove_inputs(sipp_circuit_data* cd, const uint64_t* cells, const uint64_t* values, size_t n_inputs,
                                         const uint64_t* public_inputs, uint32_t n_public_inputs, uint64_t* proof_out, size_t proof_cap,
                                         size_t* proof_len) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if ((n_inputs && (!cells || !values)) || !proof_out || !proof_len || (n_public_inputs && !public_inputs) || n_public_inputs > (1u << 24))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove inputs: null argument");
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
        unsigned int* d_conflict = reinterpret_cast<unsigned int*>(d_pairs + 2 * n_inputs);
        SIPP_CHECK_HIP(ctx, hipMemsetAsync(cd->d_wires, 0, total * 8, ctx->stream));
        if (n_inputs) {
            SIPP_CHECK_HIP(ctx, hipMemsetAsync(d_conflict, 0, 8, ctx->stream));
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_cells, cells, n_inputs * 8, hipMemcpyHostToDevice, ctx->stream));
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_values, values, n_inputs * 8, hipMemcpyHostToDevice, ctx->stream));
            const size_t want = (n_inputs + 255) / 256;
            const dim3 grid((unsigned)(want < 4096 ? want : 4096));
            hipLaunchKernelGGL(circuit_scatter_inputs_kernel, grid, dim3(256), 0, ctx->stream, cd->d_wires, d_cells, d_values, n_inputs);
            hipLaunchKernelGGL(circuit_check_inputs_kernel, grid, dim3(256), 0, ctx->stream, cd->d_wires, d_cells, d_values, n_inputs, d_conflict);
            SIPP_CHECK_HIP(ctx, hipGetLastError());
            unsigned int conflict = 0;
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(&conflict, d_conflict, sizeof conflict, hipMemcpyDeviceToHost, ctx->stream));
            SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (conflict) return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove inputs: one cell given two different values");
        }
    }
    return prove_uploaded(cd, public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
}

extern "C" int sipp_circuit_prove_words(sipp_circuit_data* cd, const uint64_t* words, size_t n_words, const uint64_t* extra, size_t n_extra,
                                        const uint64_t* public_inputs, uint32_t n_public_inputs, uint64_t* proof_out, size_t proof_cap,
                                        size_t* proof_len) {
    if (!cd) return SIPP_E_BADARG;
    sipp_ctx* ctx = cd->ctx;
    if ((n_words && !words) || (n_extra && !extra) || !proof_out || !proof_len || (n_public_inputs && !public_inputs) || n_public_inputs > (1u << 24))
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: null argument");
    if (!cd->has_map) return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: no input map set (sipp_circuit_set_input_map)");
    if (n_words != cd->map_words || n_extra != cd->map_extra)
        return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: n_words / n_extra differ from the input map's");
    const size_t total = (size_t)cd->circ.num_wires << cd->log_n, n = cd->map_n;
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    {
        // as in sipp_circuit_prove_inputs: the staging goes back before witness generation, behind the wait for the flag
        ArenaScope scope(ctx);
        uint64_t* d_staged = arena_alloc_t<uint64_t>(ctx, n_words + n_extra + 1);        // words, extra, the flag's word
        if (!d_staged) return SIPP_E_NOMEM;
        unsigned int* d_conflict = reinterpret_cast<unsigned int*>(d_staged + n_words + n_extra);
        SIPP_CHECK_HIP(ctx, hipMemsetAsync(cd->d_wires, 0, total * 8, ctx->stream));
        if (n) {
            SIPP_CHECK_HIP(ctx, hipMemsetAsync(d_conflict, 0, 8, ctx->stream));
            if (n_words) SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_staged, words, n_words * 8, hipMemcpyHostToDevice, ctx->stream));
            if (n_extra) SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d_staged + n_words, extra, n_extra * 8, hipMemcpyHostToDevice, ctx->stream));
            const uint64_t *d_cells = cd->d_map, *d_sources = cd->d_map + n;
            const size_t want = (n + 255) / 256;
            const dim3 grid((unsigned)(want < 4096 ? want : 4096));
            hipLaunchKernelGGL(circuit_scatter_words_kernel, grid, dim3(256), 0, ctx->stream, cd->d_wires, d_cells, d_sources, d_staged, n);
            hipLaunchKernelGGL(circuit_check_words_kernel, grid, dim3(256), 0, ctx->stream, cd->d_wires, d_cells, d_sources, d_staged, n, d_conflict);
            SIPP_CHECK_HIP(ctx, hipGetLastError());
            unsigned int conflict = 0;
            SIPP_CHECK_HIP(ctx, hipMemcpyAsync(&conflict, d_conflict, sizeof conflict, hipMemcpyDeviceToHost, ctx->stream));
            SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (conflict) return sipp_fail(ctx, SIPP_E_BADARG, "circuit prove words: one cell mapped to two different values");
        }
    }
    return prove_uploaded(cd, public_inputs, n_public_inputs, proof_out, proof_cap, proof_len);
}

extern "C" int sipp_circuit_verify(const sipp_circuit_data* cd, const uint64_t* proof, size_t len, int* reason) {
    if (!cd) return SIPP_E_BADARG;
    return sipp_plonk_verify_gates_lookup(proof, len, cd->cap.data(), &cd->p, &cd->fp, &cd->circ, cd->digest, cd->lookup, reason);
}
