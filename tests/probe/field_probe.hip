// tests/probe/field_probe.hip -- test-only probes of the product's field and Poseidon headers (tests/test_gpu_field_edges.py).
//
// Small elementwise kernels that INSTANTIATE the product's own headers (gl.hpp, gl_lazy.hpp, fq.hpp, poseidon.hpp, poseidon_pair.hpp)
// with the product's flags and macros, so that the code under test is the code the product kernels inline.  No arithmetic of its
// own and no inline assembly: every result comes from a header function.  One plain C entry point per family takes device pointers
// (torch tensors' data_ptr()), runs on the null stream and synchronises; the return value is the hipError_t of the launch.
//
// The Poseidon constant tables are uploaded by probe_init() from the same generated arrays as sipp_poseidon_init_constants; the
// __constant__ / __device__ symbols are this library's own, separate from libsipp_hip.so's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#define GLL_T 140
#include "gl.hpp"
#include "gl_lazy.hpp"
#include "fq.hpp"
#include "poseidon.hpp"
#include "poseidon_pair.hpp"

namespace {

__device__ __forceinline__ uint64_t gid() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
inline unsigned blocks(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// ---- gl:: (a, b, c: one u64 each per element; E2 ops read / write pairs (c0, c1)) ----
enum GlOp {
    GL_ADD, GL_SUB, GL_NEG, GL_DBL, GL_MUL, GL_MUL_NC, GL_MAD_NC, GL_ADD_NC, GL_REDUCE128_NC, GL_REDUCE96_NC, GL_INV, GL_POW, GL_ROOT,
    GL_CANON, GL_REDUCE128, GL_REDUCE96, GL_SQR, GL_MAD,
    E2_MUL = 32, E2_SQR, E2_INV, E2_POW
};

__global__ void __launch_bounds__(256) gl_kernel(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c,
                          uint64_t* __restrict__ out, uint64_t n) {
    const uint64_t i = gid();
    if (i >= n) return;
    if (op >= E2_MUL) {
        const gl::E2 x{a[2 * i], a[2 * i + 1]};
        gl::E2 r{0, 0};
        switch (op) {
            case E2_MUL: r = gl::mul(x, gl::E2{b[2 * i], b[2 * i + 1]}); break;
            case E2_SQR: r = gl::sqr(x); break;
            case E2_INV: r = gl::inv(x); break;
            case E2_POW: r = gl::pow(x, c[i]); break;
        }
        out[2 * i] = r.c0;
        out[2 * i + 1] = r.c1;
        return;
    }
    const uint64_t x = a[i];
    uint64_t r = 0;
    switch (op) {
        case GL_ADD: r = gl::add(x, b[i]); break;
        case GL_SUB: r = gl::sub(x, b[i]); break;
        case GL_NEG: r = gl::neg(x); break;
        case GL_DBL: r = gl::dbl(x); break;
        case GL_MUL: r = gl::mul(x, b[i]); break;
        case GL_MUL_NC: r = gl::mul_nc(x, b[i]); break;
        case GL_MAD_NC: r = gl::mad_nc(x, b[i], c[i]); break;
        case GL_ADD_NC: r = gl::add_nc(x, b[i]); break;
        case GL_REDUCE128_NC: r = gl::reduce128_nc(x, b[i]); break;
        case GL_REDUCE96_NC: r = gl::reduce96_nc((uint32_t)x, b[i]); break;
        case GL_INV: r = gl::inv(x); break;
        case GL_POW: r = gl::pow(x, b[i]); break;
        case GL_ROOT: r = gl::root_of_unity((unsigned)x); break;
        case GL_CANON: r = gl::canon(x); break;
        case GL_REDUCE128: r = gl::reduce128(x, b[i]); break;
        case GL_REDUCE96: r = gl::reduce96((uint32_t)x, b[i]); break;
        case GL_SQR: r = gl::sqr(x); break;
        case GL_MAD: r = gl::mad(x, b[i], c[i]); break;
    }
    out[i] = r;
}

// ---- gll:: (the hand-scheduled blocks); MUL3_NC reads three (a, b) pairs per element and writes three products ----
enum GllOp { GLL_CANON, GLL_ADD_NC, GLL_SUB_NC, GLL_MUL_NC, GLL_REDUCE96_NC, GLL_REDUCE128_NC, GLL_MUL3_NC };

__global__ void __launch_bounds__(256) gll_kernel(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t* __restrict__ out, uint64_t n) {
    const uint64_t i = gid();
    if (i >= n) return;
    if (op == GLL_MUL3_NC) {
        const uint64_t x[3] = {a[3 * i], a[3 * i + 1], a[3 * i + 2]}, y[3] = {b[3 * i], b[3 * i + 1], b[3 * i + 2]};
        uint64_t r[3];
        gll::mul3_nc(r, x, y);
        out[3 * i] = r[0];
        out[3 * i + 1] = r[1];
        out[3 * i + 2] = r[2];
        return;
    }
    const uint64_t x = a[i];
    uint64_t r = 0;
    switch (op) {
        case GLL_CANON: r = gll::canon(x); break;
        case GLL_ADD_NC: r = gll::add_nc(x, b[i]); break;
        case GLL_SUB_NC: r = gll::sub_nc(x, b[i]); break;
        case GLL_MUL_NC: r = gll::mul_nc(x, b[i]); break;
        case GLL_REDUCE96_NC: r = gll::reduce96_nc((uint32_t)x, b[i]); break;
        case GLL_REDUCE128_NC: r = gll::reduce128_nc(x, b[i]); break;
    }
    out[i] = r;
}

// ---- lazy accumulators.  Element i: start (lo, hi) = start[2 i], start[2 i + 1]; term t: x[t n + i] times y[t n + i] ----
// op 0: Acc6 (set, mac of x's halves times limbs3(y), gl::Acc6::reduce); op 1: the same sums through poseidon_pair::acc6_reduce;
// op 2: Acc160 (mac of the full products x y from zero; start unused)
__global__ void __launch_bounds__(256) acc_kernel(int op, const uint64_t* __restrict__ start, const uint64_t* __restrict__ x, const uint64_t* __restrict__ y,
                           uint32_t terms, uint64_t* __restrict__ out, uint64_t n) {
    const uint64_t i = gid();
    if (i >= n) return;
    if (op == 2) {
        gl::Acc160 acc;
        for (uint32_t t = 0; t < terms; t++) acc.mac(x[t * n + i], y[t * n + i]);
        out[i] = acc.reduce();
        return;
    }
    gl::Acc6 acc;
    acc.set((uint32_t)start[2 * i], (uint32_t)start[2 * i + 1]);
    for (uint32_t t = 0; t < terms; t++) {
        const uint64_t v = x[t * n + i];
        uint32_t l[3];
        gl::limbs3(l, y[t * n + i]);
        acc.mac((uint32_t)v, (uint32_t)(v >> 32), l);
    }
    out[i] = op == 0 ? acc.reduce() : poseidon_pair::acc6_reduce(acc);
}

// ---- fq:: (an Fq is 8 u32 words, 4 u64 per element; Fq2 ops read / write 8 u64 per element: c0 then c1) ----
enum FqOp {
    FQ_ADD, FQ_SUB, FQ_NEG, FQ_DBL, FQ_MUL, FQ_SQR, FQ_TO_MONT, FQ_FROM_MONT, FQ_INV, FQ_INV_GCD, FQ_IS_ZERO,
    FQ2_ADD = 16, FQ2_SUB, FQ2_MUL, FQ2_SQR, FQ2_INV, FQ2_INV_GCD
};

__device__ __forceinline__ fq::Fq load_fq(const uint64_t* p) {
    fq::Fq r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        r.l[2 * k] = (uint32_t)p[k];
        r.l[2 * k + 1] = (uint32_t)(p[k] >> 32);
    }
    return r;
}
__device__ __forceinline__ void store_fq(uint64_t* p, const fq::Fq& a) {
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = ((uint64_t)a.l[2 * k + 1] << 32) | a.l[2 * k];
}

__global__ void __launch_bounds__(256) fq_kernel(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t* __restrict__ out, uint64_t n) {
    const uint64_t i = gid();
    if (i >= n) return;
    if (op >= FQ2_ADD) {
        const fq::Fq2 x{load_fq(a + 8 * i), load_fq(a + 8 * i + 4)}, y{load_fq(b + 8 * i), load_fq(b + 8 * i + 4)};
        fq::Fq2 r{fq::zero(), fq::zero()};
        switch (op) {
            case FQ2_ADD: r = fq::add(x, y); break;
            case FQ2_SUB: r = fq::sub(x, y); break;
            case FQ2_MUL: r = fq::mul(x, y); break;
            case FQ2_SQR: r = fq::sqr(x); break;
            case FQ2_INV: r = fq::inv(x); break;
            case FQ2_INV_GCD: r = fq::inv_gcd(x); break;
        }
        store_fq(out + 8 * i, r.c0);
        store_fq(out + 8 * i + 4, r.c1);
        return;
    }
    const fq::Fq x = load_fq(a + 4 * i), y = load_fq(b + 4 * i);
    fq::Fq r = fq::zero();
    switch (op) {
        case FQ_ADD: r = fq::add(x, y); break;
        case FQ_SUB: r = fq::sub(x, y); break;
        case FQ_NEG: r = fq::neg(x); break;
        case FQ_DBL: r = fq::dbl(x); break;
        case FQ_MUL: r = fq::mul(x, y); break;
        case FQ_SQR: r = fq::sqr(x); break;
        case FQ_TO_MONT: r = fq::to_mont(x); break;
        case FQ_FROM_MONT: r = fq::from_mont(x); break;
        case FQ_INV: r = fq::inv(x); break;
        case FQ_INV_GCD: r = fq::inv_gcd(x); break;
        case FQ_IS_ZERO: r.l[0] = fq::is_zero(x) ? 1u : 0u; break;
    }
    store_fq(out + 4 * i, r);
}

// ---- Poseidon layers: 12 u64 per element in and out ----
// The matrix-pipe forms need every lane of the wave (MFMA ignores EXEC): whole 64-lane blocks, a lane past the end works on the last
// element again and skips the store -- the product's leaf kernel does the same.
// op 0 / 1: mds_full<false> / <true>; 2 / 3: mds_full_mfma<false> / <true> (the added constants: round `arg` of c_rc, 0 .. 30);
// 4: dense_mfma<false> of matrix `arg`; 5: dense_mfma<true> of matrix `arg`, the addend's 11 words per element from `addend`;
// 6 / 7: permute<false> / permute<true>
__global__ void __launch_bounds__(64) poseidon_kernel(int op, uint32_t arg, const uint64_t* __restrict__ in, const uint64_t* __restrict__ addend,
                                                      uint64_t* __restrict__ out, uint64_t n) {
    __shared__ uint64_t stash[11 * 64];
    const uint64_t i0 = gid(), i = i0 < n ? i0 : n - 1;
    uint64_t s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = in[12 * i + k];
    const uint64_t* rc = poseidon::c_rc + 12 * arg;
    switch (op) {
        case 0: poseidon::mds_full<false>(s, nullptr); break;
        case 1: poseidon::mds_full<true>(s, rc); break;
        case 2: poseidon::mds_full_mfma<false>(s, nullptr, poseidon::mds_a_fragment(), 0); break;
        case 3: poseidon::mds_full_mfma<true>(s, rc, poseidon::mds_a_fragment(), 0); break;
        case 4:
        case 5: {
            uint32_t lo[12], hi[12];
            uint64_t o[12];
#pragma unroll
            for (int k = 0; k < 12; k++) {
                lo[k] = (uint32_t)s[k];
                hi[k] = (uint32_t)(s[k] >> 32);
            }
            if (op == 4)
                poseidon::dense_mfma<false>(lo, hi, arg, o, nullptr, 0, 0);
            else
                poseidon::dense_mfma<true>(lo, hi, arg, o, addend + 11 * i, 1, 0);
#pragma unroll
            for (int k = 0; k < 11; k++) s[k] = o[k];
            s[11] = 0;
            break;
        }
        case 6: poseidon::permute<false>(s); break;
        case 7: poseidon::permute<true>(s, stash + threadIdx.x, 64); break;
    }
    if (i0 < n) {
#pragma unroll
        for (int k = 0; k < 12; k++) out[12 * i + k] = s[k];
    }
}

}  // namespace

extern "C" {

int probe_init() {
    hipError_t e = hipSuccess;
#define PROBE_UPLOAD(sym, arr) \
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(sym), arr, sizeof(arr))
    PROBE_UPLOAD(poseidon::c_rc, SIPP_POSEIDON_RC);
    PROBE_UPLOAD(poseidon::c_fast_first, SIPP_POSEIDON_FAST_FIRST);
    PROBE_UPLOAD(poseidon::c_fast_scalar, SIPP_POSEIDON_FAST_SCALAR);
    PROBE_UPLOAD(poseidon::c_fast_mi, SIPP_POSEIDON_FAST_MI);
    PROBE_UPLOAD(poseidon::c_fast_vs, SIPP_POSEIDON_FAST_VS);
    PROBE_UPLOAD(poseidon::c_fast_what, SIPP_POSEIDON_FAST_WHAT);
    PROBE_UPLOAD(poseidon::c_blk3, SIPP_POSEIDON_BLK3);
    PROBE_UPLOAD(poseidon::c_comb3, SIPP_POSEIDON_COMB3);
    PROBE_UPLOAD(poseidon::c_comb_c, SIPP_POSEIDON_COMB_C);
    PROBE_UPLOAD(poseidon::d_dense_a, SIPP_POSEIDON_DENSE_A);
    PROBE_UPLOAD(poseidon::c_dense_start, SIPP_POSEIDON_DENSE_START);
#undef PROBE_UPLOAD
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

int probe_dense_mats() { return SIPP_POSEIDON_DENSE_MATS; }

static int finish() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

int probe_gl(int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, uint64_t n) {
    if (n) hipLaunchKernelGGL(gl_kernel, dim3(blocks(n, 256)), dim3(256), 0, 0, op, a, b, c, out, n);
    return finish();
}

int probe_gll(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    if (n) hipLaunchKernelGGL(gll_kernel, dim3(blocks(n, 256)), dim3(256), 0, 0, op, a, b, out, n);
    return finish();
}

int probe_acc(int op, const uint64_t* start, const uint64_t* x, const uint64_t* y, uint32_t terms, uint64_t* out, uint64_t n) {
    if (n) hipLaunchKernelGGL(acc_kernel, dim3(blocks(n, 256)), dim3(256), 0, 0, op, start, x, y, terms, out, n);
    return finish();
}

int probe_fq(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    if (n) hipLaunchKernelGGL(fq_kernel, dim3(blocks(n, 256)), dim3(256), 0, 0, op, a, b, out, n);
    return finish();
}

int probe_poseidon(int op, uint32_t arg, const uint64_t* in, const uint64_t* addend, uint64_t* out, uint64_t n) {
    if (op < 0 || op > 7 || ((op == 4 || op == 5) && arg >= SIPP_POSEIDON_DENSE_MATS) || (op < 4 && arg > 30)) return (int)hipErrorInvalidValue;
    if (n) hipLaunchKernelGGL(poseidon_kernel, dim3(blocks(n, 64)), dim3(64), 0, 0, op, arg, in, addend, out, n);
    return finish();
}

}  // extern "C"
