// tests/probe/stark_probe.hip -- test-only entries to the STARK prover's two stage drivers (tests/test_gpu_stark_quotient_cases.py).
//
// Host code only: no kernel and no arithmetic of its own.  sipp_k_z_columns and sipp_k_quotient (sipp_amd/csrc/prover.hip) are reached
// by the product only through whole proofs, where every cell is the LDE of an honest trace and every challenge comes from the
// transcript; here they are called on the caller's device buffers (torch tensors' data_ptr()) and the caller's challenges.  The library
// is linked, not rebuilt: its internal entries have default visibility.  `ctx` is the handle sipp_amd.Ctx holds; the drivers enqueue on
// the ctx's stream, every entry synchronises it before it returns the driver's status code.
//
// The AIR is chosen by its INDEX in AIR_AIRS (data/air_tables.h), not through sipp_air_get: the quotient is pointwise and table_bits
// enters one constraint only, so both table variants of an AIR run at any log_n.
#include "ctx.hpp"
#include "prover.hpp"

namespace {
constexpr int N_AIRS = (int)(sizeof(AIR_AIRS) / sizeof(AIR_AIRS[0]));

int synced(sipp_ctx* ctx, int rc) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc != SIPP_OK) return rc;
    return e == hipSuccess ? SIPP_OK : SIPP_E_HIP;
}
}  // namespace

extern "C" {

int probe_air_count() { return N_AIRS; }

// name: at least 32 bytes; info[9] = kind, table_bits, n_main, checked_base, n_checked, n_aux, n_gadgets, log_rows, hardened
int probe_air_info(int i, char* name, int* info) {
    if (i < 0 || i >= N_AIRS) return -1;
    const air_spec_t& a = AIR_AIRS[i];
    strncpy(name, a.name, 31);
    name[31] = 0;
    const int v[9] = {a.kind, a.table_bits, a.n_main, a.checked_base, a.n_checked, a.n_aux, a.n_gadgets, a.log_rows, a.hardened};
    memcpy(info, v, sizeof v);
    return 0;
}

// d_lde [W][lde_stride], d_zlde [2 n_checked][lde_stride], d_aux [n_aux][2N], d_out [2][2N]: leaf order, the first 2N leaves are read
int probe_quotient(void* ctx, int air_index, uint32_t log_n, const uint64_t* d_lde, const uint64_t* d_zlde, size_t lde_stride,
                   const uint64_t* d_aux, const uint64_t* alpha, const uint64_t* beta, const uint64_t* gamma, uint64_t* d_out) {
    if (air_index < 0 || air_index >= N_AIRS) return SIPP_E_BADARG;
    sipp_ctx* c = static_cast<sipp_ctx*>(ctx);
    return synced(c, sipp_k_quotient(c, &AIR_AIRS[air_index], log_n, d_lde, d_zlde, lde_stride, d_aux, alpha, beta, gamma, d_out));
}

// a layout of the caller's: d_trace [n_main + 2 n_checked][N] (table column 0, checked columns from checked_base, then the permuted
// inputs and the permuted tables), d_zv [2 n_checked][N]
int probe_z_columns(void* ctx, int n_main, int checked_base, int n_checked, const uint64_t* d_trace, uint32_t log_n, const uint64_t* beta,
                    const uint64_t* gamma, uint64_t* d_zv) {
    air_spec_t a{};
    a.name = "probe";
    a.n_main = n_main;
    a.checked_base = checked_base;
    a.n_checked = n_checked;
    sipp_ctx* c = static_cast<sipp_ctx*>(ctx);
    return synced(c, sipp_k_z_columns(c, &a, d_trace, log_n, beta, gamma, d_zv));
}

uint32_t probe_rest_chunks(uint32_t log_n, int n_checked) { return sipp_quotient_rest_chunks(log_n, n_checked); }

}  // extern "C"
