// sipp_amd/csrc/lookup.hip -- LOOKUP TABLES by a log-derivative (LogUp) argument, the device half below the quotient: the
// multiplicities of a wire table and the running-sum columns S / U from caller-given eta, theta.  The library's
// own statement, shaped to fit the outer prover's oracles (the table in CONSTANT columns, the multiplicities in WIRES); it does not
// follow plonky2's RE / SLDC bookkeeping.
//
// Description (eight uint32 words): q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab, tag_const0.  q_look / q_tab are
// constant columns of 0 / 1 that mark looking rows and table rows.  Slot k of a looking row is the pair of wires (look_wire0 + 2k,
// + 2k + 1); slot k of a table row is the pair of constants (tab_const0 + 2k, + 2k + 1) with its multiplicity in wire tab_mult0 + k.
// tag_const0 = 0: one table.  Otherwise SEVERAL TABLES told apart by a tag: constant column tag_const0 holds the tag of every looking
// row, tag_const0 + 1 the tag of every table row (any field value), and a combination is x + eta y + eta^2 tag: a pair under another
// tag is another entry.  Every kernel that forms a combination is a template over TAGGED: the one-table instantiation is the code it
// was before the tags, the tagged one loads its row's tag once and folds eta^2 tag into theta.
//
// Layout: column-major [column][row], natural row order, like plonk.hip.  Kernels: one lane per table cell (zero), one lane per looking
// slot (binary search in the sorted index, one 64-bit atomic add on the multiplicity cell: integer additions commute, so the counts do
// not depend on the order the lanes arrive in), one lane per row and challenge for the group sums (ONE inversion per row: Montgomery's
// trick over the <= 128 group denominators), a two-level prefix SUM over the rows for S, one lane per row for the U columns.
#include "ctx.hpp"
#include "prover.hpp"
#include <algorithm>

namespace {

using plonk_desc::Lookup;
using plonk_desc::lookup_of;
using plonk_desc::MAX_CH;
constexpr uint32_t MAX_GROUPS = 128;   // groups: ceil(128 / 2) looking + ceil(128 / 2) table

// plonk_desc::lookup_check's reasons as the refusals of include/sipp_hip.h
int lookup_check(sipp_ctx* ctx, const uint32_t* w, uint32_t num_wires, uint32_t num_constants, uint32_t num_selectors, Lookup* out) {
    if (!w) return sipp_fail(ctx, SIPP_E_BADARG, "lookup: no description");
    *out = lookup_of(w);
    using R = plonk_desc::LookupReason;
    switch (plonk_desc::lookup_check(*out, num_wires, num_constants, num_selectors)) {
    case R::ok: return SIPP_OK;
    case R::too_many_slots: return sipp_fail(ctx, SIPP_E_UNSUPPORTED, "lookup: at most 128 looking slots and 128 table slots a row");
    case R::empty_with_tag: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: an empty description names no tag columns");
    case R::one_sided: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: looking slots without table slots, or the reverse");
    case R::circuit_sizes: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: malformed circuit sizes");
    case R::column_outside: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: the description names a column outside the circuit");
    case R::marker_is_selector: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: q_look and q_tab are constant columns behind the selector columns");
    case R::tag_columns: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: tag_const0 names two constant columns behind the selector columns");
    }
    return SIPP_E_BADARG;
}

// ---- multiplicities ------------------------------------------------------------------------------------------------------------------
// The index of a table: its DISTINCT canonical entries (tag, x, y) in ascending order (the tag of an untagged description is 0), each
// with the wire cell of the first slot in (row, slot) order that holds it -- that slot takes every look of the entry, the others stay 0.
struct TableIndex {
    const uint64_t *kx, *ky;   // [T] sorted
    const uint64_t* cell;      // [T] index into the wire table: (tab_mult0 + slot) * n + row
    const uint64_t* kt;        // [T] the tags; read by the tagged kernel only
    uint32_t T;
};

struct MultArgs {
    uint64_t* wires;           // [num_wires][n]
    const uint64_t* consts;    // [num_constants][n]
    uint32_t log_n;
    Lookup l;
    TableIndex ix;
    uint32_t* flag;            // != 0: a looked-up pair is in no table slot
};

__global__ void __launch_bounds__(256) lookup_zero_kernel(MultArgs a) {
    const uint32_t n = 1u << a.log_n, i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= n || gl::canon(a.consts[(size_t)a.l.q_tab * n + i]) == 0) return;
    a.wires[(size_t)(a.l.tab_mult0 + k) * n + i] = 0;
}

template <bool TAGGED>
__global__ void __launch_bounds__(256) lookup_count_kernel(MultArgs a) {
    const uint32_t n = 1u << a.log_n, i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= n || gl::canon(a.consts[(size_t)a.l.q_look * n + i]) == 0) return;
    const uint64_t x = gl::canon(a.wires[(size_t)(a.l.look_wire0 + 2 * k) * n + i]);
    const uint64_t y = gl::canon(a.wires[(size_t)(a.l.look_wire0 + 2 * k + 1) * n + i]);
    const uint64_t t = TAGGED ? gl::canon(a.consts[(size_t)a.l.tag_const0 * n + i]) : 0;      // the looking row's tag
    uint32_t lo = 0, hi = a.ix.T;                      // the first entry >= (t, x, y)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t mx = a.ix.kx[mid], my = a.ix.ky[mid];
        bool below = mx < x || (mx == x && my < y);
        if (TAGGED) {
            const uint64_t mt = a.ix.kt[mid];
            below = mt < t || (mt == t && below);
        }
        if (below) lo = mid + 1; else hi = mid;
    }
    if (lo < a.ix.T && a.ix.kx[lo] == x && a.ix.ky[lo] == y && (!TAGGED || a.ix.kt[lo] == t))
        atomicAdd(reinterpret_cast<unsigned long long*>(a.wires + a.ix.cell[lo]), 1ull);
    else
        atomicOr(a.flag, 1u);
}

// The index on the host (once per table: the table is constants): kx[T] | ky[T] | cell[T] | kt[T].  The marker columns must hold 0 / 1
int index_host(sipp_ctx* ctx, const uint64_t* d_consts, uint32_t log_n, const Lookup& l, std::vector<uint64_t>* out) {
    const size_t n = (size_t)1 << log_n;
    std::vector<uint64_t> qt(n), ql(n), tab((size_t)2 * l.n_tab * n);
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(qt.data(), d_consts + (size_t)l.q_tab * n, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(ql.data(), d_consts + (size_t)l.q_look * n, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(tab.data(), d_consts + (size_t)l.tab_const0 * n, tab.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint64_t> tag;                        // the table rows' tags
    if (l.tagged()) {
        tag.resize(n);
        SIPP_CHECK_HIP(ctx, hipMemcpyAsync(tag.data(), d_consts + (size_t)(l.tag_const0 + 1) * n, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    struct Entry { uint64_t t, x, y, cell; };
    std::vector<Entry> es;
    for (size_t i = 0; i < n; i++) {
        if (gl::canon(qt[i]) > 1 || gl::canon(ql[i]) > 1) return sipp_fail(ctx, SIPP_E_BADARG, "lookup: q_look and q_tab hold 0 or 1");
        if (gl::canon(qt[i]) == 0) continue;
        for (uint32_t k = 0; k < l.n_tab; k++)
            es.push_back(Entry{l.tagged() ? gl::canon(tag[i]) : 0, gl::canon(tab[(size_t)(2 * k) * n + i]), gl::canon(tab[(size_t)(2 * k + 1) * n + i]),
                               (size_t)(l.tab_mult0 + k) * n + i});
    }
    // stable: among equal entries the first in (row, slot) order stays in front
    std::stable_sort(es.begin(), es.end(), [](const Entry& a, const Entry& b) { return a.t != b.t ? a.t < b.t : a.x != b.x ? a.x < b.x : a.y < b.y; });
    es.erase(std::unique(es.begin(), es.end(), [](const Entry& a, const Entry& b) { return a.t == b.t && a.x == b.x && a.y == b.y; }), es.end());
    const size_t T = es.size();
    out->assign(4 * T, 0);
    for (size_t t = 0; t < T; t++) (*out)[t] = es[t].x, (*out)[T + t] = es[t].y, (*out)[2 * T + t] = es[t].cell, (*out)[3 * T + t] = es[t].t;
    return SIPP_OK;
}

int read_flag(sipp_ctx* ctx, const uint32_t* d_flag, uint32_t* h) {
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(h, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SIPP_OK;
}

// zero, count, read the flag back: the index is device memory (kx | ky | cell | kt, T each)
int multiplicities_indexed(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_consts, uint32_t log_n, const Lookup& l, const uint64_t* d_index,
                           uint32_t T) {
    ArenaScope scope(ctx, true);
    MultArgs a{};
    a.wires = d_wires; a.consts = d_consts; a.log_n = log_n; a.l = l;
    a.ix = TableIndex{d_index, d_index + T, d_index + 2 * (size_t)T, d_index + 3 * (size_t)T, T};
    a.flag = arena_alloc_t<uint32_t>(ctx, 1);
    if (!a.flag) return SIPP_E_NOMEM;
    SIPP_CHECK_HIP(ctx, hipMemsetAsync(a.flag, 0, 4, ctx->stream));
    const size_t n = (size_t)1 << log_n;
    {
        ProfScope ps(ctx, "lookup_mult");
        hipLaunchKernelGGL(lookup_zero_kernel, dim3((unsigned)((n + 255) / 256), l.n_tab), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(l.tagged() ? lookup_count_kernel<true> : lookup_count_kernel<false>, dim3((unsigned)((n + 255) / 256), l.n_look), dim3(256),
                           0, ctx->stream, a);
    }
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    uint32_t flag = 0;
    SIPP_TRY(read_flag(ctx, a.flag, &flag));
    if (flag) return sipp_fail(ctx, SIPP_E_WITNESS, "lookup: a looked-up pair is in no table slot (of its row's tag)");
    return SIPP_OK;
}

// ---- S / U ---------------------------------------------------------------------------------------------------------------------------
struct SumArgs {
    const uint64_t* wires;
    const uint64_t* consts;
    uint32_t log_n, D, Jl, Jt, C;
    Lookup l;
    uint64_t eta[MAX_CH], theta[MAX_CH];
    uint64_t* grp;             // [C][J][n]  the group sums: q_look Nl / Dl, - q_tab Nt / Dt
    uint64_t* tot;             // [C][n]     a row's sum = S(g x) - S(x)
    uint32_t* flag;            // != 0: theta hit a combination of a marked row
};

// A group's sum of 1 / d_k (looking) or m_k / e_k (table) as ONE fraction: slot by slot  N / Dn + m / d = (N d + m Dn) / (Dn d)
template <bool TAGGED>
__global__ void __launch_bounds__(256) lookup_group_kernel(SumArgs a) {
    const uint32_t n = 1u << a.log_n, i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (i >= n) return;
    const uint32_t J = a.Jl + a.Jt;
    const uint64_t eta = a.eta[c];
    uint64_t theta_l = a.theta[c], theta_t = theta_l;     // theta - eta^2 tag: all slots of a row share its tag
    if (TAGGED) {
        const uint64_t eta2 = gl::mul(eta, eta);
        theta_l = gl::sub(theta_l, gl::mul(eta2, a.consts[(size_t)a.l.tag_const0 * n + i]));
        theta_t = gl::sub(theta_t, gl::mul(eta2, a.consts[(size_t)(a.l.tag_const0 + 1) * n + i]));
    }
    const bool look = gl::canon(a.consts[(size_t)a.l.q_look * n + i]) != 0, tab = gl::canon(a.consts[(size_t)a.l.q_tab * n + i]) != 0;
    uint64_t* g = a.grp + (size_t)c * J * n + i;
    uint64_t num[MAX_GROUPS], pre[MAX_GROUPS];         // group numerators; prefix products of the group denominators
    uint64_t run = 1;
    bool hit = false;
#pragma unroll 1
    for (uint32_t j = 0; j < J; j++) {
        const bool lk = j < a.Jl;
        uint64_t N = 0, Dn = 1;
        if (lk ? look : tab) {                         // an unmarked row's step is 0: its term is 0 whatever the row holds
            const uint32_t jj = lk ? j : j - a.Jl, k1 = min((jj + 1) * a.D, lk ? a.l.n_look : a.l.n_tab);
            for (uint32_t k = jj * a.D; k < k1; k++) {
                uint64_t vx, vy, m = 1;
                if (lk) {
                    vx = a.wires[(size_t)(a.l.look_wire0 + 2 * k) * n + i];
                    vy = a.wires[(size_t)(a.l.look_wire0 + 2 * k + 1) * n + i];
                } else {
                    vx = a.consts[(size_t)(a.l.tab_const0 + 2 * k) * n + i];
                    vy = a.consts[(size_t)(a.l.tab_const0 + 2 * k + 1) * n + i];
                    m = gl::canon(a.wires[(size_t)(a.l.tab_mult0 + k) * n + i]);
                }
                const uint64_t d = gl::sub(lk ? theta_l : theta_t, gl::mad(eta, vy, gl::canon(vx)));      // theta - (x + eta y + eta^2 tag)
                hit |= d == 0;
                N = gl::add(gl::mul(N, d), lk ? Dn : gl::mul(m, Dn));
                Dn = gl::mul(Dn, d);
            }
            if (!lk) N = gl::neg(N);
        }
        if (Dn == 0) Dn = 1;                           // reported through the flag; keeps the other rows' arithmetic defined
        num[j] = N;
        pre[j] = run;
        run = gl::mul(run, Dn);
        g[(size_t)j * n] = Dn;                         // the denominator itself, for the backward sweep
    }
    if (hit) atomicOr(a.flag, 1u);
    uint64_t inv = gl::inv(run), t = 0;
#pragma unroll 1
    for (uint32_t j = J; j-- > 0;) {
        const uint64_t Dn = g[(size_t)j * n];
        const uint64_t v = gl::mul(num[j], gl::mul(inv, pre[j]));
        inv = gl::mul(inv, Dn);
        g[(size_t)j * n] = v;
        t = gl::add(t, v);
    }
    a.tot[(size_t)c * n + i] = t;
}

// U_j = S + the first j + 1 group sums, j < J - 1 (the last group closes onto S(g x))
__global__ void __launch_bounds__(256) lookup_u_kernel(const uint64_t* grp, uint64_t* out, uint32_t log_n, uint32_t J, uint32_t C) {
    const uint32_t n = 1u << log_n, i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (i >= n) return;
    uint64_t acc = out[(size_t)c * n + i];
    for (uint32_t j = 0; j + 1 < J; j++) {
        acc = gl::add(acc, grp[((size_t)c * J + j) * n + i]);
        out[((size_t)C + (size_t)c * (J - 1) + j) * n + i] = acc;
    }
}

// the chunk size and the challenges: sipp_plonk_params' own range, without the permutation argument's needs (no routed wire, no chunk cap)
int params_check(sipp_ctx* ctx, const sipp_plonk_params* p, uint32_t log_n) {
    uint32_t log_d, m;
    switch (plonk_desc::params_check(p, log_n, 0, &log_d, &m)) {
    case plonk_desc::Params::ok: return SIPP_OK;
    case plonk_desc::Params::bad_argument: return sipp_fail(ctx, SIPP_E_BADARG, "lookup: bad parameters");
    default: return sipp_fail(ctx, SIPP_E_UNSUPPORTED, "lookup: the chunk size must be a power of two in 2 .. 64, with at most 8 challenges");
    }
}

}  // namespace

uint32_t sipp_plonk_lookup_num_columns(const sipp_plonk_params* p, const uint32_t* lookup) {
    if (!p || !lookup || params_check(nullptr, p, 1) != SIPP_OK) return 0;
    const Lookup l = lookup_of(lookup);
    if (l.n_look == 0 || l.n_tab == 0 || l.n_look > plonk_desc::MAX_SLOTS || l.n_tab > plonk_desc::MAX_SLOTS) return 0;
    return l.columns(p->max_degree, p->num_challenges);
}

int sipp_plonk_lookup_multiplicities(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, uint32_t num_wires,
                                     uint32_t num_constants, uint32_t num_selectors, const uint32_t* lookup) {
    if (!ctx || !d_wires || !d_constants || log_n < 1 || log_n > 24) return ctx ? sipp_fail(ctx, SIPP_E_BADARG, "lookup: bad parameters") : SIPP_E_BADARG;
    Lookup l;
    SIPP_TRY(lookup_check(ctx, lookup, num_wires, num_constants, num_selectors, &l));
    if (l.empty()) return SIPP_OK;
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    ArenaScope scope(ctx, true);
    std::vector<uint64_t> h;
    SIPP_TRY(index_host(ctx, d_constants, log_n, l, &h));
    uint64_t* d = arena_alloc_t<uint64_t>(ctx, std::max<size_t>(1, h.size()));
    if (!d) return SIPP_E_NOMEM;
    if (!h.empty()) SIPP_CHECK_HIP(ctx, hipMemcpyAsync(d, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `h` is host memory
    return multiplicities_indexed(ctx, d_wires, d_constants, log_n, l, d, (uint32_t)(h.size() / 4));
}

int sipp_plonk_lookup_sums(sipp_ctx* ctx, const uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, uint32_t num_wires,
                           uint32_t num_constants, uint32_t num_selectors, const sipp_plonk_params* p, const uint32_t* lookup,
                           const uint64_t* etas, const uint64_t* thetas, uint64_t* d_out) {
    if (!ctx || !d_wires || !d_constants || !etas || !thetas) return ctx ? sipp_fail(ctx, SIPP_E_BADARG, "lookup: bad parameters") : SIPP_E_BADARG;
    SIPP_TRY(params_check(ctx, p, log_n));
    Lookup l;
    SIPP_TRY(lookup_check(ctx, lookup, num_wires, num_constants, num_selectors, &l));
    if (l.empty()) return SIPP_OK;                   // no columns
    if (!d_out) return sipp_fail(ctx, SIPP_E_BADARG, "lookup: bad parameters");
    return sipp_lookup_sums(ctx, d_wires, d_constants, log_n, p, l, etas, thetas, d_out);
}

// (a non-empty description the caller has validated against the circuit, parameters in params_check's range)
int sipp_lookup_sums(sipp_ctx* ctx, const uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, const sipp_plonk_params* p, const Lookup& l,
                     const uint64_t* etas, const uint64_t* thetas, uint64_t* d_out) {
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    ArenaScope scope(ctx, true);
    const size_t n = (size_t)1 << log_n;
    const uint32_t C = p->num_challenges;
    SumArgs a{};
    a.wires = d_wires; a.consts = d_constants; a.log_n = log_n; a.D = p->max_degree; a.C = C; a.l = l;
    a.Jl = l.Jl(a.D); a.Jt = l.Jt(a.D);
    const uint32_t J = a.Jl + a.Jt;
    for (uint32_t c = 0; c < C; c++) { a.eta[c] = gl::canon(etas[c]); a.theta[c] = gl::canon(thetas[c]); }
    a.grp = arena_alloc_t<uint64_t>(ctx, (size_t)C * J * n);
    a.tot = arena_alloc_t<uint64_t>(ctx, (size_t)C * n);
    a.flag = arena_alloc_t<uint32_t>(ctx, 1);
    if (!a.grp || !a.tot || !a.flag) return SIPP_E_NOMEM;
    SIPP_CHECK_HIP(ctx, hipMemsetAsync(a.flag, 0, 4, ctx->stream));
    {
        ProfScope ps(ctx, "lookup_sums");
        hipLaunchKernelGGL(l.tagged() ? lookup_group_kernel<true> : lookup_group_kernel<false>, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0,
                           ctx->stream, a);
        hipLaunchKernelGGL(sipp_scan_kernel<ScanSum>, dim3(C), dim3(1024), 0, ctx->stream, a.tot, d_out, log_n);
        hipLaunchKernelGGL(lookup_u_kernel, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, ctx->stream, a.grp, d_out, log_n, J, C);
    }
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    uint32_t flag = 0;
    SIPP_TRY(read_flag(ctx, a.flag, &flag));
    if (flag) return sipp_fail(ctx, SIPP_E_WITNESS, "lookup: theta hit a looking or table combination (a vanishing denominator)");
    return SIPP_OK;
}

// ---- the lookup terms of the quotient ------------------------------------------------------------------------------------------------
// A kernel of its own over the quotient coset, run behind plonk_quotient_kernel and in front of the coset iNTT: it ADDS
// Z_H^-1 sum_k alpha^(n0 + k) term_k to the values that kernel wrote.  A circuit without lookups never launches it, and
// plonk_quotient_kernel's code does not know of it.  Terms, in the order of the one reduce_with_powers list: L_0(x) S_c(x) for every
// challenge, then challenge by challenge the J chain terms  (U_j - U_(j-1)) Dl - q_look Nl,  (U_j - U_(j-1)) Dt + q_tab Nt.
namespace {
struct LqArgs {
    const uint64_t* wl;       // [num_wires][stride]  leaf order
    const uint64_t* cl;       // [num_constants][stride]
    const uint64_t* sl;       // [C J][stride]  S_0 .. S_(C-1), then the U's challenge by challenge
    size_t stride;
    uint32_t log_n, rate_bits, log_d, D, C, Jl, Jt;
    Lookup l;
    uint64_t eta[MAX_CH], theta[MAX_CH], alpha[MAX_CH], apow0[MAX_CH];   // apow0 = alpha^(terms in front)
    uint64_t w_nd, n_field;
    uint64_t zh[64], zh_inv[64];
    uint64_t* qv;             // [C][n D]
};

template <bool TAGGED>
__global__ void __launch_bounds__(256) lookup_quotient_kernel(LqArgs a) {
    const uint32_t lq = a.log_n + a.log_d, nd = 1u << lq, pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= nd) return;
    const uint32_t L = a.log_n + a.rate_bits;
    const uint32_t i = gl::bitrev(pos, lq);                              // coset index: x = 7 w^i
    const uint32_t nat = gl::bitrev(pos, L);
    const uint32_t pos_next = gl::bitrev((nat + (1u << a.rate_bits)) & ((1u << L) - 1), L);   // g x
    const uint64_t x = gl::mul(gl::GEN, gl::pow(a.w_nd, i));
    const uint64_t zh = a.zh[i & (a.D - 1)], zhi = a.zh_inv[i & (a.D - 1)];
    const uint64_t l0 = gl::mul(zh, gl::inv(gl::mul(a.n_field, gl::sub(x, 1))));
    const uint32_t C = a.C, J = a.Jl + a.Jt;
    uint64_t acc[MAX_CH], apow[MAX_CH];
#pragma unroll
    for (uint32_t c = 0; c < MAX_CH; c++) acc[c] = 0, apow[c] = a.apow0[c];
    auto push = [&](uint64_t term) {
#pragma unroll
        for (uint32_t c = 0; c < MAX_CH; c++)
            if (c < C) {
                acc[c] = gl::add(acc[c], gl::mul(apow[c], term));
                apow[c] = gl::mul(apow[c], a.alpha[c]);
            }
    };
    for (uint32_t c = 0; c < C; c++) push(gl::mul(l0, a.sl[(size_t)c * a.stride + pos]));
    const uint64_t ql = a.cl[(size_t)a.l.q_look * a.stride + pos], qt = a.cl[(size_t)a.l.q_tab * a.stride + pos];
    for (uint32_t c = 0; c < C; c++) {
        const uint64_t eta = a.eta[c];
        uint64_t theta_l = a.theta[c], theta_t = theta_l;     // theta - eta^2 tag(x): the tag columns' polynomials on the coset
        if (TAGGED) {                                         // (88 VGPRs against 74 without the tags, held or read per challenge)
            const uint64_t eta2 = gl::mul(eta, eta);
            theta_l = gl::sub(theta_l, gl::mul(eta2, a.cl[(size_t)a.l.tag_const0 * a.stride + pos]));
            theta_t = gl::sub(theta_t, gl::mul(eta2, a.cl[(size_t)(a.l.tag_const0 + 1) * a.stride + pos]));
        }
        uint64_t prev = a.sl[(size_t)c * a.stride + pos];
        for (uint32_t j = 0; j < J; j++) {
            const bool lk = j < a.Jl;
            const uint32_t jj = lk ? j : j - a.Jl, k1 = min((jj + 1) * a.D, lk ? a.l.n_look : a.l.n_tab);
            uint64_t N = 0, Dn = 1;
            for (uint32_t k = jj * a.D; k < k1; k++) {
                uint64_t vx, vy, m = 1;
                if (lk) {
                    vx = a.wl[(size_t)(a.l.look_wire0 + 2 * k) * a.stride + pos];
                    vy = a.wl[(size_t)(a.l.look_wire0 + 2 * k + 1) * a.stride + pos];
                } else {
                    vx = a.cl[(size_t)(a.l.tab_const0 + 2 * k) * a.stride + pos];
                    vy = a.cl[(size_t)(a.l.tab_const0 + 2 * k + 1) * a.stride + pos];
                    m = a.wl[(size_t)(a.l.tab_mult0 + k) * a.stride + pos];
                }
                const uint64_t d = gl::sub(lk ? theta_l : theta_t, gl::mad(eta, vy, vx));
                N = gl::add(gl::mul(N, d), lk ? Dn : gl::mul(m, Dn));
                Dn = gl::mul(Dn, d);
            }
            const uint64_t next = j + 1 == J ? a.sl[(size_t)c * a.stride + pos_next] : a.sl[((size_t)C + (size_t)c * (J - 1) + j) * a.stride + pos];
            const uint64_t sd = gl::mul(gl::sub(next, prev), Dn);
            push(lk ? gl::sub(sd, gl::mul(ql, N)) : gl::add(sd, gl::mul(qt, N)));
            prev = next;
        }
    }
    for (uint32_t c = 0; c < C; c++) {
        uint64_t* q = a.qv + (size_t)c * nd + pos;
        *q = gl::add(*q, gl::mul(acc[c], zhi));
    }
}
}  // namespace

// ---- what plonk.hip and circuit_data.hip call (ctx.hpp) ------------------------------------------------------------------------------
int sipp_lookup_check(sipp_ctx* ctx, const uint32_t* lookup, uint32_t num_wires, uint32_t num_constants, uint32_t num_selectors, Lookup* out) {
    return lookup_check(ctx, lookup, num_wires, num_constants, num_selectors, out);
}

int sipp_lookup_index_host(sipp_ctx* ctx, const uint64_t* d_constants, uint32_t log_n, const Lookup& l, std::vector<uint64_t>* out) {
    return index_host(ctx, d_constants, log_n, l, out);
}

int sipp_lookup_multiplicities_indexed(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, const Lookup& l,
                                       const uint64_t* d_index, uint32_t n_index) {
    return multiplicities_indexed(ctx, d_wires, d_constants, log_n, l, d_index, n_index);
}

// (the caller has validated the description against the circuit and the parameters; log_d = log2(max_degree) <= rate_bits)
int sipp_lookup_quotient_terms(sipp_ctx* ctx, const uint64_t* d_wires_lde, const uint64_t* d_consts_lde, const uint64_t* d_sums_lde, uint32_t log_n,
                               uint32_t rate_bits, uint32_t log_d, const sipp_plonk_params* p, const Lookup& l, const uint64_t* etas,
                               const uint64_t* thetas, const uint64_t* alphas, uint64_t terms_in_front, uint64_t* d_qv) {
    const size_t n = (size_t)1 << log_n;
    LqArgs a{};
    a.wl = d_wires_lde; a.cl = d_consts_lde; a.sl = d_sums_lde; a.stride = n << rate_bits;
    a.log_n = log_n; a.rate_bits = rate_bits; a.log_d = log_d; a.D = p->max_degree; a.C = p->num_challenges;
    a.l = l;
    a.Jl = l.Jl(a.D); a.Jt = l.Jt(a.D);
    for (uint32_t c = 0; c < a.C; c++) {
        a.eta[c] = gl::canon(etas[c]); a.theta[c] = gl::canon(thetas[c]); a.alpha[c] = gl::canon(alphas[c]);
        a.apow0[c] = gl::pow(a.alpha[c], terms_in_front);
    }
    a.w_nd = gl::root_of_unity(log_n + log_d);
    a.n_field = (uint64_t)n;
    sipp_coset_zh(log_n, log_d, a.zh, a.zh_inv);
    a.qv = d_qv;
    const size_t nd = n << log_d;
    {
        ProfScope ps(ctx, "lookup_quotient");
        hipLaunchKernelGGL(a.l.tagged() ? lookup_quotient_kernel<true> : lookup_quotient_kernel<false>, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0,
                           ctx->stream, a);
    }
    SIPP_CHECK_HIP(ctx, hipGetLastError());
    return SIPP_OK;
}
