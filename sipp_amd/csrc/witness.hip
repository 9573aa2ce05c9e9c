// sipp_amd/csrc/witness.hip -- the gates' WITNESS GENERATORS of the outer plonky2 proof on the device:
// plonky2's prove() (reference src/verifier_circuit.rs:253 `data.prove(pw)`) begins with generate_partial_witness (iop/generator.rs), where
// every gate instance's SimpleGenerator computes the wires its constraints determine.  plonky2 @ InternetMaximalism/plonky2 541e127 is not
// vendored: the gate families and their generators follow the recalled upstream gates (gates/arithmetic_base.rs, base_sum.rs, constant.rs,
// public_input.rs, random_access.rs, reducing.rs, poseidon.rs; plonky2_u32 gates/arithmetic_u32.rs) in the layouts the caller passes as
// data (include/sipp_hip.h, sipp_plonk_generator); the checker is oracle/plonk_gates.c (orc_plonk_generate_witness) and the numpy
// generator of tools/plonk_synth.py.
//
// Layout: the wire table [num_wires][N] the prover reads next, natural row order; one LANE PER ROW, one launch per generator; a lane whose
// selector cell does not hold the generator's gate index leaves at once.  Consecutive lanes = consecutive rows of one column: every load
// and store is coalesced; nothing is staged.  The Poseidon generators are the only ones with real arithmetic (the naive 30-round form: the
// S-box INPUTS of every round are wires, so the lazy partial-round form of the hash kernels does not apply): 12 x 12 small-constant
// products per round on exactly accumulated 32-bit halves, one reduction per output.  The partial-round S-box input is element 0 of the
// naive state; upstream's fast partial rounds change the basis of elements 1 .. 11 only, so they write the same values into those wires.
// SIPP_GEN_POSEIDON_SWAP is upstream's PoseidonGate with its swap wire (a Merkle-path step): delta_i = swap (in[4+i] - in[i]) goes to its
// wires, the permutation runs on (in[i] + delta_i, in[4+i] - delta_i, in[8 .. 12)).
// The FRI fold's families (recalled gates/arithmetic_extension.rs, exponentiation.rs, coset_interpolation.rs) work over F[X]/(X^2 - W), W
// passed as data: SIPP_GEN_ARITHMETIC_EXT, SIPP_GEN_EXPONENTIATION, and SIPP_GEN_COSET_INTERPOLATION, the barycentric evaluation of the
// polynomial through n = 2^s values on the coset shift * <g> at a point, in chunks whose partial states are wires.
// FRI's initial combination (recalled gates/reducing_extension.rs, and gadgets/arithmetic_extension.rs div_add_extension with its
// QuotientGeneratorExtension) adds SIPP_GEN_REDUCING_EXT, the reduction of extension coefficients, and SIPP_GEN_QUOTIENT_EXT, which fills
// the multiplicand of an ArithmeticExtension-shaped row from its output: the one generator here that inverts.
// The recursive evaluation of the Poseidon gate (recalled gates/poseidon_mds.rs) adds SIPP_GEN_POSEIDON_MDS, the linear layer on twelve
// extension elements: a case of run_generator on one lane, wherever the row runs.
// SIPP_GEN_LOOKUP is the library's own (no upstream gate): a looking row of the lookup argument (lookup.hip) takes its y cells from a dense
// table in the constant columns, y = f(x) by address, no index; also one lane, wherever the row runs.
// SIPP's transcript in the outer circuit (recalled plonky2_u32 gates/arithmetic_u32.rs, add_many_u32.rs; sipp_amd/nonnative.py) adds
// SIPP_GEN_U32_ARITHMETIC, SIPP_GEN_U32_ADD_MANY and SIPP_GEN_NONNATIVE, the reduction and the inverse of eight u32 limbs modulo a modulus
// that is data: one lane per row, and only in kernel instantiations of their own (run_u32_generator, the U32 template flag).
// SIPP_GEN_RANDOM (blinding rows) is NOT computed here: its cells depend on no other cell and cost a whole permutation per eight wires, so
// blind.hip fills them with a kernel of its own that both entry points launch first; in run_generator the kind does nothing.
#include "ctx.hpp"
#include "poseidon_constants.h"
#include <mutex>

namespace {

__constant__ uint64_t w_rc[360];
__constant__ uint32_t w_mds_circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
constexpr uint32_t MDS_DIAG0 = 8;

// the interpolation domain: the powers of the primitive root of order 16 (x_i of the order-n subgroup = entry i * 16 / n), and 1 / 2^s
__constant__ uint64_t w_om16[16] = {0x1ull, 0xefffffff00000001ull, 0xfffffffeff000001ull, 0xffffffff00000ull, 0x1000000000000ull, 0x1000ull,
                                    0xfffffeff00000101ull, 0xffffffef00000001ull, 0xffffffff00000000ull, 0x1000000000000000ull, 0x1000000ull,
                                    0xffefffff00100001ull, 0xfffeffff00000001ull, 0xfffffffefffff001ull, 0xffffffff00ull, 0x1000000000ull};
__constant__ uint64_t w_ninv[5] = {0x1ull, 0x7fffffff80000001ull, 0xbfffffff40000001ull, 0xdfffffff20000001ull, 0xefffffff10000001ull};

// F[X]/(X^2 - nr)
struct X2 {
    uint64_t a, b;
};
__device__ __forceinline__ X2 xmul(X2 x, X2 y, uint64_t nr) {
    return X2{gl::add(gl::mul(x.a, y.a), gl::mul(nr, gl::mul(x.b, y.b))), gl::add(gl::mul(x.a, y.b), gl::mul(x.b, y.a))};
}
__device__ __forceinline__ X2 xadd(X2 x, X2 y) { return X2{gl::add(x.a, y.a), gl::add(x.b, y.b)}; }
// (x.a - x.b X) inv(x.a^2 - nr x.b^2); gl::inv(0) = 0: zero, and an element of zero norm under a residue nr, give (0, 0)
__device__ __forceinline__ X2 xinv(X2 x, uint64_t nr) {
    const uint64_t ni = gl::inv(gl::sub(gl::mul(x.a, x.a), gl::mul(nr, gl::mul(x.b, x.b))));
    return X2{gl::mul(x.a, ni), gl::mul(gl::sub(0, x.b), ni)};
}

struct GenArgs {
    uint64_t* wires;
    const uint64_t* consts;
    uint32_t n;
    sipp_plonk_generator g;
    uint64_t pih[4];
};

// row i holds generator g: its selector cell carries g's gate index
__device__ __forceinline__ bool row_holds(const uint64_t* consts, uint32_t n, uint32_t i, const sipp_plonk_generator& g) {
    return consts[(size_t)g.selector_index * n + i] == g.row;
}

__host__ __device__ __forceinline__ bool is_poseidon(uint32_t kind) { return kind == SIPP_GEN_POSEIDON || kind == SIPP_GEN_POSEIDON_SWAP; }

__device__ __forceinline__ uint64_t pow7(uint64_t x) {
    const uint64_t x2 = gl::mul(x, x), x4 = gl::mul(x2, x2);
    return gl::mul(gl::mul(x4, x2), x);
}

// out = M s: M[r][c] = circ[(c - r) mod 12] + [r = c = 0] 8, entries below 2^6: the halves accumulate exactly (12 products below 2^38)
__device__ __forceinline__ void mds(uint64_t (&s)[12]) {
    uint64_t out[12];
#pragma unroll
    for (int r = 0; r < 12; r++) {
        uint64_t al = 0, ah = 0;
#pragma unroll
        for (int c = 0; c < 12; c++) {
            const uint32_t k = w_mds_circ[(c - r + 12) % 12] + ((r == 0 && c == 0) ? MDS_DIAG0 : 0);
            al += (uint64_t)(uint32_t)s[c] * k;
            ah += (s[c] >> 32) * k;
        }
        // al + 2^32 ah as (hi32, lo): ah < 2^42
        const uint64_t lo = al + (ah << 32);
        const uint32_t hi = (uint32_t)(ah >> 32) + (lo < al ? 1u : 0u);
        out[r] = gl::reduce96(hi, lo);
    }
#pragma unroll
    for (int r = 0; r < 12; r++) s[r] = out[r];
}

// the 30 rounds of the naive permutation on s, every S-box input of rounds 1 .. 29 into its wire (sbox + 12 (r - 1) + i, sbox + 36 + (r - 4),
// sbox + 58 + 12 (r - 26) + i), the outputs into out .. out + 12
template <class WireRef>
__device__ __forceinline__ void poseidon_rounds(WireRef& W, uint64_t (&s)[12], uint32_t out, uint32_t sb) {
#pragma unroll 1
    for (uint32_t rnd = 0; rnd < 30; rnd++) {
        const bool full = rnd < 4 || rnd >= 26;
#pragma unroll
        for (int l = 0; l < 12; l++) s[l] = gl::add(s[l], w_rc[12 * rnd + l]);
        if (full) {
            const uint32_t base = rnd < 4 ? sb + 12 * (rnd - 1) : sb + 58 + 12 * (rnd - 26);
#pragma unroll
            for (int l = 0; l < 12; l++) {
                if (rnd) W(base + l) = s[l];
                s[l] = pow7(s[l]);
            }
        } else {
            W(sb + 36 + (rnd - 4)) = s[0];
            s[0] = pow7(s[0]);
        }
        mds(s);
    }
#pragma unroll
    for (int l = 0; l < 12; l++) W(out + l) = s[l];
}

// SIPP_GEN_POSEIDON_MDS on row i: twelve extension elements, element c limb l at p + 2 c + l; M is over the base field, so each limb is one
// product.  The limbs are field values, whatever word they hold (the exact half sums take any 64-bit word); the outputs are canonical.
// Every kernel here inlines it, and mds() with its twelve outputs live cost the row-local kernel a wave per SIMD inlined (76 VGPRs) and
// more out of line (102): so the outputs are taken ONE AT A TIME, in a loop the compiler must not unroll, the coefficients of row r read
// from constant memory by a wave-uniform index (scalar loads).  The same exact half-product sum as mds(): the 24 written cells never
// meet the 24 read ones (layout_ok), so an output is stored as soon as it is reduced.
__device__ __forceinline__ void poseidon_mds_row(uint64_t* wires, uint32_t n, uint32_t i, uint32_t in, uint32_t out) {
#pragma unroll 1
    for (uint32_t l = 0; l < 2; l++) {
        uint64_t s[12];
#pragma unroll
        for (int c = 0; c < 12; c++) s[c] = wires[(size_t)(in + 2 * c + l) * n + i];
#pragma unroll 1
        for (uint32_t r = 0; r < 12; r++) {
            uint64_t al = 0, ah = 0;
#pragma unroll
            for (uint32_t c = 0; c < 12; c++) {
                const uint32_t at = c + 12 - r, k = w_mds_circ[at >= 12 ? at - 12 : at] + ((r == 0 && c == 0) ? MDS_DIAG0 : 0);
                al += (uint64_t)(uint32_t)s[c] * k;
                ah += (s[c] >> 32) * k;
            }
            const uint64_t lo = al + (ah << 32);
            wires[(size_t)(out + 2 * r + l) * n + i] = gl::reduce96((uint32_t)(ah >> 32) + (lo < al ? 1u : 0u), lo);
        }
    }
}

// SIPP_GEN_LOOKUP on row i: entry t of a dense table (x = t) sits in table row row0 + t / n_tab, slot t % n_tab; row0 and T are the row's
// own constants.  An x outside the table (x >= T, or an entry row at or behind n) writes y = 0: the lookup argument refuses the row.
// 64-bit row arithmetic: row0, T and x are any field values.  `span` = the entries whose row is inside the circuit, so x < min(T, span)
// says both conditions and bounds x below n n_tab < 2^58 before it is divided.
__device__ __forceinline__ void lookup_row(uint64_t* wires, const uint64_t* consts, uint32_t n, uint32_t i, const sipp_plonk_generator& g) {
    const uint32_t lw = g.p[0], n_look = g.p[1], tc = g.p[2], n_tab = g.p[3], bc = g.p[4];
    const uint64_t row0 = gl::canon(consts[(size_t)bc * n + i]), T = gl::canon(consts[(size_t)(bc + 1) * n + i]);
    if (T == 0) return;                                       // a plain looking row: both coordinates are the circuit's
    const uint64_t span = row0 < n ? (uint64_t)(n - (uint32_t)row0) * n_tab : 0;
    const uint64_t lim = T < span ? T : span;
#pragma unroll 1
    for (uint32_t k = 0; k < n_look; k++) {
        const uint64_t x = gl::canon(wires[(size_t)(lw + 2 * k) * n + i]);
        uint64_t y = 0;
        if (x < lim) {
            const uint64_t q = x / n_tab;                     // < n - row0
            const uint32_t slot = (uint32_t)(x - q * n_tab);
            y = gl::canon(consts[(size_t)(tc + 2 * slot + 1) * n + (uint32_t)(row0 + q)]);
        }
        wires[(size_t)(lw + 2 * k + 1) * n + i] = y;
    }
}

// one generator on one row
__device__ __forceinline__ void run_generator(uint64_t* wires, const uint64_t* consts, uint32_t n, uint32_t i, const sipp_plonk_generator& g,
                                              const uint64_t* pih) {
    auto W = [&](uint32_t j) -> uint64_t& { return wires[(size_t)j * n + i]; };
    auto K = [&](uint32_t j) -> uint64_t { return consts[(size_t)j * n + i]; };
    switch (g.kind) {
    case SIPP_GEN_ARITHMETIC: {
        const uint64_t c0 = K(g.p[1]), c1 = K(g.p[2]);
        for (uint32_t k = 0; k < g.p[0]; k++)
            W(4 * k + 3) = gl::add(gl::mul(c0, gl::mul(W(4 * k), W(4 * k + 1))), gl::mul(c1, W(4 * k + 2)));
        break;
    }
    case SIPP_GEN_BASE_SPLIT: {
        const uint64_t v = W(0), mask = (1ull << g.p[1]) - 1;
        for (uint32_t l = 0; l < g.p[0]; l++) W(1 + l) = (v >> (g.p[1] * l)) & mask;
        break;
    }
    case SIPP_GEN_CONSTANT:
        for (uint32_t l = 0; l < g.p[0]; l++) W(l) = K(g.p[1] + l);
        break;
    case SIPP_GEN_PUBLIC_INPUT:
        for (uint32_t l = 0; l < 4; l++) W(l) = pih[l];
        break;
    case SIPP_GEN_U32_MUL_ADD:
        for (uint32_t op = 0; op < g.p[0]; op++) {
            const uint32_t b = g.p[1] * op, L = g.p[2];
            // the inputs are u32 values (range-checked where they were produced): the full result fits 64 bits
            const uint64_t full = (W(b) & 0xffffffffull) * (W(b + 1) & 0xffffffffull) + (W(b + 2) & 0xffffffffull);
            const uint64_t half[2] = {full & 0xffffffffull, full >> 32};
            W(b + 3) = half[0];
            W(b + 4) = half[1];
            for (uint32_t h = 0; h < 2; h++)
                for (uint32_t l = 0; l < L; l++) W(b + 5 + L * h + l) = (half[h] >> (2 * l)) & 3;
        }
        break;
    case SIPP_GEN_RANDOM_ACCESS:
        for (uint32_t cp = 0; cp < g.p[0]; cp++) {
            const uint32_t b = g.p[1] * cp, bits = g.p[2], len = 1u << bits;
            const uint32_t idx = (uint32_t)W(b) & (len - 1);
            W(b + 1) = W(b + 2 + idx);
            for (uint32_t l = 0; l < bits; l++) W(b + 2 + len + l) = (idx >> l) & 1;
        }
        break;
    case SIPP_GEN_REDUCING: {
        const uint32_t Kc = g.p[0];
        const uint64_t nr = g.p[1], al0 = W(0), al1 = W(1);
        uint64_t a0 = W(2), a1 = W(3);
        for (uint32_t l = 0; l < Kc; l++) {
            const uint64_t n0 = gl::add(gl::add(gl::mul(a0, al0), gl::mul(gl::mul(a1, al1), nr)), W(4 + l));
            const uint64_t n1 = gl::add(gl::mul(a0, al1), gl::mul(a1, al0));
            W(4 + Kc + 2 * l) = n0;
            W(5 + Kc + 2 * l) = n1;
            a0 = n0, a1 = n1;
        }
        break;
    }
    case SIPP_GEN_POSEIDON: {
        uint64_t s[12];
#pragma unroll
        for (int l = 0; l < 12; l++) s[l] = W(g.p[0] + l);
        poseidon_rounds(W, s, g.p[1], g.p[2]);
        break;
    }
    case SIPP_GEN_POSEIDON_SWAP: {
        const uint32_t in = g.p[0], dl = g.p[4];
        uint64_t s[12];
#pragma unroll
        for (int l = 0; l < 12; l++) s[l] = W(in + l);
        const uint64_t b = W(g.p[3]);       // any field value: booleanity is the constraints' job
#pragma unroll
        for (int l = 0; l < 4; l++) {
            const uint64_t d = gl::mul(b, gl::sub(s[4 + l], s[l]));
            W(dl + l) = d;
            s[l] = gl::add(s[l], d);
            s[4 + l] = gl::sub(s[4 + l], d);
        }
        poseidon_rounds(W, s, g.p[1], g.p[2]);
        break;
    }
    case SIPP_GEN_ARITHMETIC_EXT: {
        const uint64_t c0 = K(g.p[1]), c1 = K(g.p[2]), nr = g.p[3];
        for (uint32_t k = 0; k < g.p[0]; k++) {
            const uint32_t b = 8 * k;
            const X2 m = xmul(X2{W(b), W(b + 1)}, X2{W(b + 2), W(b + 3)}, nr);
            W(b + 6) = gl::add(gl::mul(c0, m.a), gl::mul(c1, W(b + 4)));
            W(b + 7) = gl::add(gl::mul(c0, m.b), gl::mul(c1, W(b + 5)));
        }
        break;
    }
    case SIPP_GEN_EXPONENTIATION: {
        const uint32_t nb = g.p[0];
        const uint64_t base = W(0);
        uint64_t prev = 1;
        for (uint32_t k = 0; k < nb; k++) {
            const uint64_t bit = W(nb - k);     // any field value: bit base + 1 - bit
            prev = gl::mul(gl::sqr(prev), gl::sub(gl::add(gl::mul(bit, base), 1), bit));
            W(2 + nb + k) = prev;
        }
        W(1 + nb) = prev;
        break;
    }
    case SIPP_GEN_COSET_INTERPOLATION: {
        const uint32_t s = g.p[0], d = g.p[1], np = 1u << s, ni = (np - 2) / (d - 1), start = 5 + 2 * np;
        const uint64_t nr = g.p[2], si = gl::inv(W(0));
        const X2 sh{gl::mul(W(1 + 2 * np), si), gl::mul(W(2 + 2 * np), si)};
        W(start + 4 * ni) = sh.a;
        W(start + 4 * ni + 1) = sh.b;
        X2 e{0, 0}, q{1, 0};
        uint32_t bound = d < np ? d : np, c = 0;
        for (uint32_t k = 0; k < np; k++) {
            const uint64_t x = w_om16[k << (4 - s)], wt = gl::mul(x, w_ninv[s]);
            const X2 t{gl::sub(sh.a, x), sh.b}, vw{gl::mul(W(1 + 2 * k), wt), gl::mul(W(2 + 2 * k), wt)};
            e = xadd(xmul(e, t, nr), xmul(vw, q, nr));
            q = xmul(q, t, nr);
            if (k + 1 == bound && k + 1 < np) {     // a chunk ends before the last point: its state is a pair of wires
                W(start + 2 * c) = e.a;
                W(start + 2 * c + 1) = e.b;
                W(start + 2 * ni + 2 * c) = q.a;
                W(start + 2 * ni + 2 * c + 1) = q.b;
                c++;
                bound += d - 1;
            }
        }
        W(3 + 2 * np) = e.a;
        W(4 + 2 * np) = e.b;
        break;
    }
    case SIPP_GEN_REDUCING_EXT: {
        const uint32_t Kc = g.p[0];
        const uint64_t nr = g.p[1];
        const X2 al{W(0), W(1)};
        X2 acc{W(2), W(3)};
        for (uint32_t l = 0; l < Kc; l++) {
            acc = xadd(xmul(acc, al, nr), X2{W(4 + 2 * l), W(5 + 2 * l)});
            W(4 + 2 * Kc + 2 * l) = acc.a;
            W(5 + 2 * Kc + 2 * l) = acc.b;
        }
        break;
    }
    case SIPP_GEN_QUOTIENT_EXT: {
        const uint64_t c0 = K(g.p[1]), c1 = K(g.p[2]), nr = g.p[3];
        for (uint32_t k = 0; k < g.p[0]; k++) {
            const uint32_t b = 8 * k;
            // (out - c1 c) inv(c0 a): a zero denominator writes (0, 0), and the row's constraints hold only if out = c1 c
            const X2 num{gl::sub(W(b + 6), gl::mul(c1, W(b + 4))), gl::sub(W(b + 7), gl::mul(c1, W(b + 5)))};
            const X2 m = xmul(num, xinv(X2{gl::mul(c0, W(b)), gl::mul(c0, W(b + 1))}, nr), nr);
            W(b + 2) = m.a;
            W(b + 3) = m.b;
        }
        break;
    }
    case SIPP_GEN_BASE_SUM: {
        // Horner from the top limb: the limbs are field values, whatever they hold (mad takes any 64-bit word)
        const uint64_t base = 1ull << g.p[1];
        uint64_t acc = 0;
        for (uint32_t l = g.p[0]; l-- > 0;) acc = gl::mad(acc, base, W(1 + l));
        W(0) = acc;
        break;
    }
    case SIPP_GEN_POSEIDON_MDS:
        poseidon_mds_row(wires, n, i, g.p[0], g.p[1]);
        break;
    case SIPP_GEN_LOOKUP:
        lookup_row(wires, consts, n, i, g);
        break;
    case SIPP_GEN_RANDOM:      // blinding rows depend on no cell: blind.hip has filled them before the first launch of either entry point
    default: break;
    }
}

// ---- the u32 and nonnative families (SIPP_GEN_U32_ARITHMETIC, _U32_ADD_MANY, _NONNATIVE) -----------------------------------------------------
// They are not cases of run_generator: only the U32 instantiations of the kernels below carry this code, and the host picks those for
// a generator list that holds one of the three kinds.  A 256-bit value is eight u32 limbs, least significant first, in an array that is
// only ever indexed by unrolled loops (registers, no scratch); the loops over bits and over Euclid's steps stay rolled.
__host__ __device__ __forceinline__ bool is_u32_family(uint32_t kind) { return kind >= SIPP_GEN_U32_ARITHMETIC && kind <= SIPP_GEN_NONNATIVE; }

template <int NL>
__device__ __forceinline__ bool big_is_zero(const uint32_t (&a)[NL]) {
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) acc |= a[k];
    return acc == 0;
}
__device__ __forceinline__ bool big_is_one(const uint32_t (&a)[8]) {
    uint32_t acc = a[0] ^ 1u;
#pragma unroll
    for (int k = 1; k < 8; k++) acc |= a[k];
    return acc == 0;
}
// d = a - b mod 2^256 -> the borrow
__device__ __forceinline__ uint32_t big_sub(uint32_t (&d)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
    uint32_t br = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)a[k] - b[k] - br;
        d[k] = (uint32_t)t;
        br = (uint32_t)(t >> 63);
    }
    return br;
}
// d = a + b mod 2^256 -> the carry
__device__ __forceinline__ uint32_t big_add(uint32_t (&d)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t t = (uint64_t)a[k] + b[k] + c;
        d[k] = (uint32_t)t;
        c = (uint32_t)(t >> 32);
    }
    return c;
}
// a = 2 a + in mod 2^(32 NL) -> the bit shifted out
template <int NL>
__device__ __forceinline__ uint32_t big_shl1(uint32_t (&a)[NL], uint32_t in) {
#pragma unroll
    for (int k = 0; k < NL; k++) {
        const uint32_t out = a[k] >> 31;
        a[k] = (a[k] << 1) | in;
        in = out;
    }
    return in;
}
// a = (a + 2^256 top) / 2
__device__ __forceinline__ void big_shr1(uint32_t (&a)[8], uint32_t top) {
#pragma unroll
    for (int k = 0; k < 7; k++) a[k] = (a[k] >> 1) | (a[k + 1] << 31);
    a[7] = (a[7] >> 1) | (top << 31);
}
// num (32 NL bits, consumed) = quotient m + rem, rem < m, for m != 0: schoolbook division bit by bit from the top.  q keeps the
// quotient's low 256 bits (all of it for NL = 8; for NL = 16 the callers' quotients are below 2^256).  rem < m before a step, so
// 2 rem + bit < 2 m: where the shift carries out of 256 bits the difference still fits them.
template <int NL>
__device__ __forceinline__ void big_divmod(uint32_t (&num)[NL], const uint32_t (&m)[8], uint32_t (&q)[8], uint32_t (&rem)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) q[k] = 0, rem[k] = 0;
#pragma unroll 1
    for (uint32_t it = 0; it < 32 * NL; it++) {
        const uint32_t top = big_shl1<8>(rem, big_shl1<NL>(num, 0));
        uint32_t d[8];
        const uint32_t take = top | (big_sub(d, rem, m) ^ 1u);
#pragma unroll
        for (int k = 0; k < 8; k++) rem[k] = take ? d[k] : rem[k];
        (void)big_shl1<8>(q, take);
    }
}
// a^-1 mod m for an odd m > 1 and a < m, by the binary extended Euclid: x1 a = u and x2 a = v (mod m) throughout, v stays odd, and
// every step halves u -- after subtracting the smaller odd value where u is odd -- so bits(u) + bits(v) falls by one at least: at
// most 512 steps.  At u = 0, v = gcd(a, m).  -> whether the gcd is 1; inv = x2 then.
__device__ __forceinline__ bool big_inverse(const uint32_t (&a)[8], const uint32_t (&m)[8], uint32_t (&inv)[8]) {
    uint32_t u[8], v[8], x1[8], d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) u[k] = a[k], v[k] = m[k], x1[k] = k == 0, inv[k] = 0;
#pragma unroll 1
    while (!big_is_zero<8>(u)) {
        if (u[0] & 1u) {
            if (big_sub(d, u, v)) {                          // u < v: the two pairs change places
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint32_t tu = u[k], tx = x1[k];
                    u[k] = v[k], v[k] = tu, x1[k] = inv[k], inv[k] = tx;
                }
            }
            (void)big_sub(u, u, v);
            if (big_sub(x1, x1, inv)) (void)big_add(x1, x1, m);
        }
        big_shr1(u, 0);
        uint32_t c = 0;
        if (x1[0] & 1u) c = big_add(x1, x1, m);              // (x1 + m) / 2 < m
        big_shr1(x1, c);
    }
    return big_is_one(v);
}

// SIPP_GEN_NONNATIVE on row i: x at x0 and the modulus m at m0, eight u32 limbs each (operands by their low 32 bits); result, quotient
// and slack = m - 1 - result, eight limbs each, at out0.  op 0: result = x mod m, quotient = x / m.  op 1: result = (x mod m)^-1 mod m,
// quotient = k with x result = k m + 1.  m = 0, or under op 1 an even m, m = 1 or gcd(x, m) != 1: 24 zeros.
__device__ __forceinline__ void nonnative_row(uint64_t* wires, uint32_t n, uint32_t i, const sipp_plonk_generator& g) {
    const uint32_t op = g.p[0], x0 = g.p[1], m0 = g.p[2], out0 = g.p[3];
    uint32_t x[8], m[8], res[8], quo[8], slack[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        x[k] = (uint32_t)wires[(size_t)(x0 + k) * n + i];
        m[k] = (uint32_t)wires[(size_t)(m0 + k) * n + i];
        res[k] = 0, quo[k] = 0, slack[k] = 0;
    }
    bool ok = !big_is_zero<8>(m);
    if (op == 1) ok = ok && (m[0] & 1u) && !big_is_one(m);
    if (ok) {
        uint32_t num[8];
#pragma unroll
        for (int k = 0; k < 8; k++) num[k] = x[k];
        big_divmod<8>(num, m, quo, res);
        if (op == 1) {
            uint32_t inv[8];
            ok = big_inverse(res, m, inv);
            if (ok) {
                // x inv - 1 over sixteen limbs (inv >= 1 and x >= 1 here), then its exact quotient by m
                uint32_t pr[16];
#pragma unroll
                for (int k = 0; k < 16; k++) pr[k] = 0;
#pragma unroll
                for (int a = 0; a < 8; a++) {
                    uint64_t c = 0;
#pragma unroll
                    for (int b = 0; b < 8; b++) {
                        const uint64_t t = (uint64_t)x[a] * inv[b] + pr[a + b] + c;
                        pr[a + b] = (uint32_t)t;
                        c = t >> 32;
                    }
                    pr[a + 8] = (uint32_t)c;
                }
                uint32_t br = 1;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const uint32_t t = pr[k] - br;
                    br = br & (pr[k] == 0);
                    pr[k] = t;
                }
                big_divmod<16>(pr, m, quo, res);
            }
#pragma unroll
            for (int k = 0; k < 8; k++) res[k] = ok ? inv[k] : 0, quo[k] = ok ? quo[k] : 0;
        }
    }
    if (ok) {                                                   // m - 1 - result: result < m
        uint32_t br = 1;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint64_t t = (uint64_t)m[k] - res[k] - br;
            slack[k] = (uint32_t)t;
            br = (uint32_t)(t >> 63);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        wires[(size_t)(out0 + k) * n + i] = res[k];
        wires[(size_t)(out0 + 8 + k) * n + i] = quo[k];
        wires[(size_t)(out0 + 16 + k) * n + i] = slack[k];
    }
}

// one generator of the three kinds on one row
__device__ __forceinline__ void run_u32_generator(uint64_t* wires, uint32_t n, uint32_t i, const sipp_plonk_generator& g) {
    auto W = [&](uint32_t j) -> uint64_t& { return wires[(size_t)j * n + i]; };
    constexpr uint64_t M32 = 0xffffffffull;
    switch (g.kind) {
    case SIPP_GEN_U32_ARITHMETIC:
        for (uint32_t op = 0; op < g.p[0]; op++) {
            const uint32_t b = g.p[1] * op, L = g.p[2];
            // a b + c <= (2^32 - 1)^2 + 2^32 - 1 = p - 1: (lo, hi) is the one split of a canonical value
            const uint64_t full = (W(b) & M32) * (W(b + 1) & M32) + (W(b + 2) & M32);
            const uint64_t half[2] = {full & M32, full >> 32};
            W(b + 3) = half[0];
            W(b + 4) = half[1];
            W(b + 5) = gl::inv(M32 - half[1]);               // inv(0) = 0: hi all ones, where the constraint needs lo = 0
            for (uint32_t h = 0; h < 2; h++)
                for (uint32_t l = 0; l < L; l++) W(b + 6 + L * h + l) = (half[h] >> (2 * l)) & 3;
        }
        break;
    case SIPP_GEN_U32_ADD_MANY:
        for (uint32_t op = 0; op < g.p[0]; op++) {
            const uint32_t b = g.p[1] * op, A = g.p[2], C = g.p[3];
            uint64_t sum = W(b + A) & M32;                      // the carry-in
            for (uint32_t k = 0; k < A; k++) sum += W(b + k) & M32;
            const uint64_t lo = sum & M32, carry = sum >> 32;
            W(b + A + 1) = lo;
            W(b + A + 2) = carry;
            for (uint32_t l = 0; l < 16; l++) W(b + A + 3 + l) = (lo >> (2 * l)) & 3;
            for (uint32_t l = 0; l < C; l++) W(b + A + 19 + l) = (carry >> (2 * l)) & 3;
        }
        break;
    case SIPP_GEN_NONNATIVE:
        nonnative_row(wires, n, i, g);
        break;
    default: break;
    }
}

// SIPP_GEN_REDUCING / SIPP_GEN_REDUCING_EXT on the sixteen lanes of a row (all lanes of the wave call it; act = the row holds the
// generator, ext = its coefficients are extension elements): lane l owns the chunk of m = ceil(K / 16) consecutive coefficients from
// l m as the affine map acc -> acc M + C, (M, C) = (alpha^len, Horner of the chunk from 0).  Under (M1, C1) (M2, C2) = (M1 M2, C1 M2 + C2),
// associative with the identity (1, 0), an inclusive scan in four steps of two independent extension products gives every lane the map
// of everything up to its chunk's end; the lane takes the map before its chunk from its neighbour, applies it to the old accumulator
// and replays its chunk, storing the accumulators: about 2 m + 5 dependent products where one lane walks K.  Shuffles of width 16, no
// LDS, no barrier.  The coefficients are read twice (the second time from cache): K has no bound that registers could hold.
__device__ __forceinline__ void reducing_lanes(uint64_t* wires, uint32_t n, uint32_t i, uint32_t l, bool act, bool ext, uint32_t Kc,
                                               uint64_t nr) {
    auto W = [&](uint32_t j) -> uint64_t& { return wires[(size_t)j * n + i]; };
    const uint32_t m = (Kc + 15) / 16, first = l * m, cnt = !act || first >= Kc ? 0 : (Kc - first < m ? Kc - first : m);
    auto coef = [&](uint32_t j) -> X2 { return ext ? X2{W(4 + 2 * j), W(5 + 2 * j)} : X2{W(4 + j), 0}; };
    const X2 al = act ? X2{W(0), W(1)} : X2{0, 0};
    X2 M{1, 0}, C{0, 0};
    for (uint32_t t = 0; t < cnt; t++) {
        C = xadd(xmul(C, al, nr), coef(first + t));
        M = xmul(M, al, nr);
    }
#pragma unroll
    for (uint32_t off = 1; off < 16; off <<= 1) {
        const X2 Ml{__shfl_up((unsigned long long)M.a, off, 16), __shfl_up((unsigned long long)M.b, off, 16)};
        const X2 Cl{__shfl_up((unsigned long long)C.a, off, 16), __shfl_up((unsigned long long)C.b, off, 16)};
        if (l >= off) {
            C = xadd(xmul(Cl, M, nr), C);
            M = xmul(Ml, M, nr);
        }
    }
    X2 Me{__shfl_up((unsigned long long)M.a, 1, 16), __shfl_up((unsigned long long)M.b, 1, 16)};
    X2 Ce{__shfl_up((unsigned long long)C.a, 1, 16), __shfl_up((unsigned long long)C.b, 1, 16)};
    if (l == 0) Me = X2{1, 0}, Ce = X2{0, 0};
    if (!cnt) return;
    const uint32_t accs = ext ? 4 + 2 * Kc : 4 + Kc;
    X2 acc = xadd(xmul(X2{W(2), W(3)}, Me, nr), Ce);
    for (uint32_t t = 0; t < cnt; t++) {
        acc = xadd(xmul(acc, al, nr), coef(first + t));
        W(accs + 2 * (first + t)) = acc.a;
        W(accs + 2 * (first + t) + 1) = acc.b;
    }
}

// SIPP_GEN_COSET_INTERPOLATION on the sixteen lanes of a row (all lanes of the wave call it; act = the row holds the generator): lane k
// owns point k as the pair (t_k, v_k w_k) = (shifted - x_k, value_k w_k).  Under (T1, E1) (T2, E2) = (T1 T2, E1 T2 + T1 E2), which is
// associative with the identity (1, 0), the product of the first k + 1 pairs is (q, e) after point k: an inclusive scan in four steps
// of three extension products gives every chunk boundary at once, where one lane walks 3 n dependent products.  A row's lanes are one
// DPP row: shuffles of width 16, no LDS, no barrier.  Every lane of the row computes inv(shift) (lanes of a wave share their
// instructions: one lane alone would take the same time); lanes >= n carry the identity.
__device__ __forceinline__ void interpolation_lanes(uint64_t* wires, uint32_t n, uint32_t i, uint32_t l, bool act, uint32_t s, uint32_t d,
                                                    uint64_t nr) {
    auto W = [&](uint32_t j) -> uint64_t& { return wires[(size_t)j * n + i]; };
    const uint32_t np = act ? 1u << s : 0, ni = act ? (np - 2) / (d - 1) : 0, start = 5 + 2 * np;
    X2 T{1, 0}, E{0, 0};
    if (act) {
        const uint64_t si = gl::inv(W(0));
        const X2 sh{gl::mul(W(1 + 2 * np), si), gl::mul(W(2 + 2 * np), si)};
        if (l == 0) {
            W(start + 4 * ni) = sh.a;
            W(start + 4 * ni + 1) = sh.b;
        }
        if (l < np) {
            const uint64_t x = w_om16[l << (4 - s)], wt = gl::mul(x, w_ninv[s]);
            T = X2{gl::sub(sh.a, x), sh.b};
            E = X2{gl::mul(W(1 + 2 * l), wt), gl::mul(W(2 + 2 * l), wt)};
        }
    }
#pragma unroll
    for (uint32_t off = 1; off < 16; off <<= 1) {
        const X2 Tl{__shfl_up((unsigned long long)T.a, off, 16), __shfl_up((unsigned long long)T.b, off, 16)};
        const X2 El{__shfl_up((unsigned long long)E.a, off, 16), __shfl_up((unsigned long long)E.b, off, 16)};
        if (l >= off) {
            E = xadd(xmul(El, T, nr), xmul(Tl, E, nr));
            T = xmul(Tl, T, nr);
        }
    }
    if (l >= np) return;
    if (l == np - 1) {
        W(3 + 2 * np) = E.a;
        W(4 + 2 * np) = E.b;
    } else if (l + 1 >= d && (l + 1 - d) % (d - 1) == 0) {     // the last point of a chunk that is not the last
        const uint32_t c = (l + 1 - d) / (d - 1);
        W(start + 2 * c) = E.a;
        W(start + 2 * c + 1) = E.b;
        W(start + 2 * ni + 2 * c) = T.a;
        W(start + 2 * ni + 2 * c + 1) = T.b;
    }
}

__global__ void __launch_bounds__(256) plonk_witness_kernel(GenArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = a.n;
    if (i >= n) return;
    if (!row_holds(a.consts, n, i, a.g)) return;
    run_generator(a.wires, a.consts, n, i, a.g, a.pih);
}

// the row-local launch of a generator of the u32 and nonnative families
__global__ void __launch_bounds__(256) plonk_witness_u32_kernel(GenArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = a.n;
    if (i >= n) return;
    if (!row_holds(a.consts, n, i, a.g)) return;
    run_u32_generator(a.wires, n, i, a.g);
}

// ---- level by level -------------------------------------------------------------------------------------------------------------------
// A circuit's generators travel by value in the kernel arguments (scalar loads by a wave-uniform index).  Up to NARROW_GENS the struct
// is the one every circuit had before the ceiling rose; a circuit with more takes the same kernels over the MAX_GENS struct (1104 bytes
// of arguments: under the 4 KiB limit), so that a circuit at or below NARROW_GENS launches what it always launched.
constexpr uint32_t NARROW_GENS = 16, MAX_GENS = 32;
constexpr uint32_t COOP_BELOW_ROWS = 16384;   // levels with fewer rows than this leave SIMDs empty with one lane per row
template <uint32_t NG>
struct LevelArgsT {
    uint64_t* wires;
    const uint64_t* consts;
    uint32_t n, n_gens;
    const uint32_t* rows;     // the level's rows
    uint32_t count;
    int* err;
    uint64_t pih[4];
    sipp_plonk_generator g[NG];
};
using LevelArgs = LevelArgsT<NARROW_GENS>;
using LevelArgsWide = LevelArgsT<MAX_GENS>;

// one lane per row of the level; the row runs the generator whose selector value it holds (the lanes of a wave may hold different gates:
// the families are short except Poseidon, whose rows a schedule keeps together)
// U32 (here and in the two kernels below): the circuit has a generator of the u32 and nonnative families, whose code no other
// instantiation carries; a row of theirs is one lane's work on every path.
template <bool U32, class Args>
__global__ void __launch_bounds__(64) plonk_witness_level_kernel(Args a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.count) return;
    const uint32_t i = a.rows[k];
    if (i >= a.n) {
        *a.err = 1;
        return;
    }
    for (uint32_t q = 0; q < a.n_gens; q++)
        if (row_holds(a.consts, a.n, i, a.g[q])) {
            if constexpr (U32) {
                if (is_u32_family(a.g[q].kind)) {
                    run_u32_generator(a.wires, a.n, i, a.g[q]);
                    continue;
                }
            }
            run_generator(a.wires, a.consts, a.n, i, a.g[q], a.pih);
        }
}

// THIN levels (a hash chain's link: a few hundred to a few thousand rows) are latency-bound -- one lane walking a whole permutation is
// ~23 k dependent instructions.  Here a row gets SIXTEEN lanes (four rows per wave): lane l < 12 owns state element l of a Poseidon row,
// S-boxes side by side, the MDS layer through LDS (every lane reads the twelve elements of its row and accumulates its own output from
// exact 32-bit halves) -- ~3.5 k instructions deep; the short families run on lane 0 of their row's group.  One wave per block: the two
// barriers per round cost nothing.

// a lane's place in the two kernels below: group grp of the block's four, lane l of its sixteen, row i of the table.  ok is false, and
// i = 0, for a group past the level's end and for a row outside the table, which raises the error flag.  (The arguments are scalars:
// a reference to the kernel's LevelArgs cost either kernel four VGPRs.)
struct CoopRow {
    uint32_t grp, l, i;
    bool ok;
};
__device__ __forceinline__ CoopRow coop_row(const uint32_t* rows, uint32_t count, uint32_t n, int* err) {
    const uint32_t grp = threadIdx.x >> 4, l = threadIdx.x & 15, k = blockIdx.x * 4 + grp;
    bool ok = k < count;
    uint32_t i = ok ? rows[k] : 0;
    if (ok && i >= n) {
        if (l == 0) *err = 1;
        ok = false;
        i = 0;
    }
    return CoopRow{grp, l, i, ok};
}

// the 30 rounds on the sixteen lanes of row i, the one copy both kernels below run (all lanes of the block call it; act = the row is a
// Poseidon row and l < 12): lane l starts from s, state element l behind the row's prelude, and stores its S-box inputs (the wires of
// poseidon_rounds) and its output; lanes 12 .. 15 shadow element 0 and never store.  sh: the block's LDS tile, twelve words per group.
// The exact half-product sum is written here, in mds() and in poseidon_mds_row(): one helper for all changed mds()'s register allocation.
__device__ __forceinline__ void poseidon_lanes(uint64_t* wires, uint32_t n, uint32_t i, uint32_t grp, uint32_t l, bool act, uint64_t s,
                                               uint32_t out, uint32_t sb, uint64_t (&sh)[4][12]) {
    const uint32_t e = l < 12 ? l : 0;
    uint32_t coef[12];                                        // this lane's row of the MDS matrix
#pragma unroll
    for (int c = 0; c < 12; c++) coef[c] = w_mds_circ[(c + 12 - e) % 12] + ((e == 0 && c == 0) ? MDS_DIAG0 : 0);
#pragma unroll 1
    for (uint32_t rnd = 0; rnd < 30; rnd++) {
        const bool full = rnd < 4 || rnd >= 26;
        s = gl::add(s, w_rc[12 * rnd + e]);
        if (full || e == 0) {
            if (act && rnd) {
                const uint32_t w = full ? (rnd < 4 ? sb + 12 * (rnd - 1) : sb + 58 + 12 * (rnd - 26)) + e : sb + 36 + (rnd - 4);
                wires[(size_t)w * n + i] = s;
            }
            s = pow7(s);
        }
        if (l < 12) sh[grp][l] = s;
        __syncthreads();
        uint64_t al = 0, ah = 0;
#pragma unroll
        for (int c = 0; c < 12; c++) {
            const uint64_t v = sh[grp][c];
            al += (uint64_t)(uint32_t)v * coef[c];
            ah += (v >> 32) * coef[c];
        }
        const uint64_t lo = al + (ah << 32);
        s = gl::reduce96((uint32_t)(ah >> 32) + (lo < al ? 1u : 0u), lo);
        __syncthreads();
    }
    if (act) wires[(size_t)(out + e) * n + i] = s;
}

// the circuit's one Poseidon generator a.g[pos] (pos = -1: none) on the sixteen lanes, its parameters block-uniform
template <bool U32, class Args>
__global__ void __launch_bounds__(64) plonk_witness_level_coop_kernel(Args a, int pos) {
    __shared__ uint64_t sh[4][12];
    const CoopRow row = coop_row(a.rows, a.count, a.n, a.err);
    const uint32_t grp = row.grp, l = row.l, i = row.i, n = a.n;
    bool is_pos = false;
    if (row.ok) {
        if (pos >= 0) is_pos = row_holds(a.consts, n, i, a.g[pos]);
        if (l == 0)
            for (uint32_t q = 0; q < a.n_gens; q++)
                if ((int)q != pos && row_holds(a.consts, n, i, a.g[q])) {
                    if constexpr (U32) {
                        if (is_u32_family(a.g[q].kind)) {
                            run_u32_generator(a.wires, n, i, a.g[q]);
                            continue;
                        }
                    }
                    run_generator(a.wires, a.consts, n, i, a.g[q], a.pih);
                }
    }
    if (pos < 0 || !__syncthreads_or(is_pos)) return;        // block-uniform: no Poseidon row among the four
    const uint32_t in = a.g[pos].p[0], out = a.g[pos].p[1], sb = a.g[pos].p[2];
    const bool act = is_pos && l < 12;
    poseidon_lanes(a.wires, n, i, grp, l, act, act ? a.wires[(size_t)(in + l) * n + i] : 0, out, sb, sh);
}

// The same sixteen lanes per row when the circuit has a swap generator or more than one Poseidon layout: every row gets its own
// Poseidon-family generator (the last one whose selector value it holds; any other match runs on lane 0 first), so one level may mix
// layouts and the two kinds.  On a swap row lanes 0 .. 7 read their element and its partner, lanes 0 .. 3 store the deltas.  (The
// per-row parameters cost the single-generator case above ~15 % of its level time, so that case keeps its own kernel.)
// INTERP: the circuit has a SIPP_GEN_COSET_INTERPOLATION generator; a row that holds it spreads its points over its sixteen lanes
// (interpolation_lanes) unless one_lane (SIPP_ROUTE_WITNESS_INTERP_ONE_LANE) leaves it to lane 0 with the short families.
// REDUCE: the circuit has a SIPP_GEN_REDUCING_EXT or SIPP_GEN_QUOTIENT_EXT generator (FRI's initial combination, whose reducing rows are
// a query's longest chain); a row that holds SIPP_GEN_REDUCING or _REDUCING_EXT spreads its coefficients over its sixteen lanes
// (reducing_lanes) unless reduce_one_lane (SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE).  It implies INTERP's code: an interpolation generator
// may or may not be there.
template <bool INTERP, bool REDUCE, bool U32, class Args>
__global__ void __launch_bounds__(64) plonk_witness_level_coop_rows_kernel(Args a, bool one_lane, bool reduce_one_lane) {
    __shared__ uint64_t sh[4][12];
    const CoopRow row = coop_row(a.rows, a.count, a.n, a.err);
    const uint32_t grp = row.grp, l = row.l, i = row.i, n = a.n;
    int pq = -1, iq = -1, rq = -1;                            // this row's Poseidon-family generator, its sixteen-lane interpolation / reduction
    uint32_t in = 0, out = 0, sb = 0, sw = 0, dl = 0, is = 1, id = 2, inr = 0, rk = 0, rnr = 0;
    bool swp = false, rext = false;
    if (row.ok) {
        for (uint32_t q = 0; q < a.n_gens; q++) {             // uniform loop: the parameters are picked, never indexed per lane
            if (is_poseidon(a.g[q].kind) && row_holds(a.consts, n, i, a.g[q])) {
                pq = (int)q;
                in = a.g[q].p[0], out = a.g[q].p[1], sb = a.g[q].p[2], sw = a.g[q].p[3], dl = a.g[q].p[4];
                swp = a.g[q].kind == SIPP_GEN_POSEIDON_SWAP;
            }
            if (INTERP && !one_lane && a.g[q].kind == SIPP_GEN_COSET_INTERPOLATION && row_holds(a.consts, n, i, a.g[q]))
                iq = (int)q, is = a.g[q].p[0], id = a.g[q].p[1], inr = a.g[q].p[2];
            if (REDUCE && !reduce_one_lane && (a.g[q].kind == SIPP_GEN_REDUCING || a.g[q].kind == SIPP_GEN_REDUCING_EXT) &&
                row_holds(a.consts, n, i, a.g[q]))
                rq = (int)q, rk = a.g[q].p[0], rnr = a.g[q].p[1], rext = a.g[q].kind == SIPP_GEN_REDUCING_EXT;
        }
        if (l == 0)
            for (uint32_t q = 0; q < a.n_gens; q++)
                if ((int)q != pq && (int)q != iq && (int)q != rq && row_holds(a.consts, n, i, a.g[q])) {
                    if constexpr (U32) {
                        if (is_u32_family(a.g[q].kind)) {
                            run_u32_generator(a.wires, n, i, a.g[q]);
                            continue;
                        }
                    }
                    run_generator(a.wires, a.consts, n, i, a.g[q], a.pih);
                }
    }
    if (INTERP && __syncthreads_or(iq >= 0)) interpolation_lanes(a.wires, n, i, l, iq >= 0, is, id, inr);   // block-uniform
    if (REDUCE && __syncthreads_or(rq >= 0)) reducing_lanes(a.wires, n, i, l, rq >= 0, rext, rk, rnr);      // block-uniform
    const bool is_pos = pq >= 0;
    if (!__syncthreads_or(is_pos)) return;                    // block-uniform: no Poseidon row among the four
    const bool act = is_pos && l < 12;
    uint64_t s = act ? a.wires[(size_t)(in + l) * n + i] : 0;
    if (swp && l < 8) {                                       // (in[j] + d_j, in[4+j] - d_j), d_j = swap (in[4+j] - in[j])
        const uint32_t j = l & 3;
        const uint64_t lhs = a.wires[(size_t)(in + j) * n + i], rhs = a.wires[(size_t)(in + 4 + j) * n + i];
        const uint64_t d = gl::mul(a.wires[(size_t)sw * n + i], gl::sub(rhs, lhs));
        s = l < 4 ? gl::add(lhs, d) : gl::sub(rhs, d);
        if (l < 4) a.wires[(size_t)(dl + j) * n + i] = d;
    }
    poseidon_lanes(a.wires, n, i, grp, l, act, s, out, sb, sh);
}

__global__ void __launch_bounds__(256) plonk_witness_copy_kernel(uint64_t* wires, const uint64_t* src, const uint64_t* dst, uint32_t count,
                                                                 uint64_t cells, int* err) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const uint64_t s = src[k], d = dst[k];
    if (s >= cells || d >= cells) {
        *err = 1;
        return;
    }
    wires[d] = wires[s];
}

// the wires a generator reads or writes stay inside the table; constant columns inside the constants
bool layout_ok(const sipp_plonk_generator& g, uint32_t num_wires, uint32_t num_constants) {
    if (g.selector_index >= num_constants) return false;
    const uint64_t nw = num_wires;
    switch (g.kind) {
    case SIPP_GEN_ARITHMETIC: return 4ull * g.p[0] <= nw && g.p[1] < num_constants && g.p[2] < num_constants;
    case SIPP_GEN_BASE_SPLIT:
    case SIPP_GEN_BASE_SUM: return 1ull + g.p[0] <= nw && g.p[1] >= 1 && g.p[1] <= 32 && (uint64_t)g.p[0] * g.p[1] <= 64;
    case SIPP_GEN_CONSTANT: return g.p[0] <= nw && (uint64_t)g.p[1] + g.p[0] <= num_constants;
    case SIPP_GEN_PUBLIC_INPUT: return 4 <= nw;
    case SIPP_GEN_U32_MUL_ADD: return g.p[2] <= 16 && g.p[1] >= 5 + 2 * g.p[2] && (uint64_t)g.p[0] * g.p[1] <= nw;
    case SIPP_GEN_RANDOM_ACCESS: return g.p[2] >= 1 && g.p[2] <= 6 && g.p[1] >= 2 + (1u << g.p[2]) + g.p[2] && (uint64_t)g.p[0] * g.p[1] <= nw;
    case SIPP_GEN_REDUCING: return 4ull + 3ull * g.p[0] <= nw;
    case SIPP_GEN_POSEIDON: return (uint64_t)g.p[0] + 12 <= nw && (uint64_t)g.p[1] + 12 <= nw && (uint64_t)g.p[2] + 106 <= nw;
    case SIPP_GEN_ARITHMETIC_EXT: return g.p[0] >= 1 && 8ull * g.p[0] <= nw && g.p[1] < num_constants && g.p[2] < num_constants && g.p[3] != 0;
    case SIPP_GEN_EXPONENTIATION: return g.p[0] >= 1 && g.p[0] <= 64 && 2ull + 2ull * g.p[0] <= nw;
    case SIPP_GEN_COSET_INTERPOLATION: {
        if (g.p[0] < 1 || g.p[0] > 4 || g.p[1] < 2 || g.p[2] == 0) return false;
        const uint64_t np = 1ull << g.p[0], ni = (np - 2) / (g.p[1] - 1);
        return 5 + 2 * np + 4 * ni + 2 <= nw;
    }
    case SIPP_GEN_REDUCING_EXT: return g.p[0] >= 1 && 4ull + 4ull * g.p[0] <= nw && g.p[1] != 0;
    case SIPP_GEN_QUOTIENT_EXT: return g.p[0] >= 1 && 8ull * g.p[0] <= nw && g.p[1] < num_constants && g.p[2] < num_constants && g.p[3] != 0;
    case SIPP_GEN_POSEIDON_MDS: {
        const uint64_t in = g.p[0], out = g.p[1];
        return in + 24 <= nw && out + 24 <= nw && (in + 24 <= out || out + 24 <= in);
    }
    case SIPP_GEN_LOOKUP:
        return g.p[1] >= 1 && g.p[3] >= 1 && (uint64_t)g.p[0] + 2ull * g.p[1] <= nw && (uint64_t)g.p[2] + 2ull * g.p[3] <= num_constants &&
               (uint64_t)g.p[4] + 1 < num_constants;
    case SIPP_GEN_RANDOM: return (uint64_t)g.p[0] + g.p[1] <= nw;
    case SIPP_GEN_U32_ARITHMETIC: return g.p[2] <= 16 && g.p[1] >= 6 + 2 * g.p[2] && (uint64_t)g.p[0] * g.p[1] <= nw;
    case SIPP_GEN_U32_ADD_MANY:
        return g.p[2] >= 1 && g.p[2] <= 32 && g.p[3] <= 16 && g.p[1] >= g.p[2] + 19 + g.p[3] && (uint64_t)g.p[0] * g.p[1] <= nw;
    case SIPP_GEN_NONNATIVE: {
        // the 24 written cells must not meet the 16 read ones
        const uint64_t x0 = g.p[1], m0 = g.p[2], out0 = g.p[3];
        if (g.p[0] > 1 || x0 + 8 > nw || m0 + 8 > nw || out0 + 24 > nw) return false;
        return (out0 + 24 <= x0 || x0 + 8 <= out0) && (out0 + 24 <= m0 || m0 + 8 <= out0);
    }
    case SIPP_GEN_POSEIDON_SWAP: {
        // written cells (out, sbox, delta) must not meet the read cells (in, swap): the two launch paths read and write in different orders
        const uint64_t in = g.p[0], out = g.p[1], sb = g.p[2], sw = g.p[3], dl = g.p[4];
        if (in + 12 > nw || out + 12 > nw || sb + 106 > nw || sw + 1 > nw || dl + 4 > nw) return false;
        auto meet = [](uint64_t x, uint64_t lx, uint64_t y, uint64_t ly) { return x < y + ly && y < x + lx; };
        const uint64_t wr[3][2] = {{out, 12}, {sb, 106}, {dl, 4}};
        for (const auto& w : wr)
            if (meet(w[0], w[1], in, 12) || meet(w[0], w[1], sw, 1)) return false;
        return true;
    }
    default: return false;
    }
}

const char* gen_name(uint32_t kind) {
    static const char* names[] = {"", "witness_arithmetic", "witness_base_split", "witness_constant", "witness_public_input", "witness_u32",
                                  "witness_random_access", "witness_reducing", "witness_poseidon", "witness_poseidon_swap",
                                  "witness_arithmetic_ext", "witness_exponentiation", "witness_coset_interpolation",
                                  "witness_reducing_ext", "witness_quotient_ext", "witness_base_sum", "witness_poseidon_mds",
                                  "witness_lookup", "witness_random", "witness_u32_arithmetic", "witness_u32_add_many",
                                  "witness_nonnative"};
    return kind <= SIPP_GEN_NONNATIVE ? names[kind] : "witness";
}

}  // namespace

// argument checks shared by both entry points; uploads this translation unit's round constants when a Poseidon generator is there
static int witness_prepare(sipp_ctx* ctx, const uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, uint32_t num_wires,
                           uint32_t num_constants, const sipp_plonk_generator* gens, size_t n_gens, const uint64_t* public_inputs_hash,
                           const sipp_blinding* blind) {
    if (!d_wires || !d_constants || (!gens && n_gens) || log_n < 1 || log_n > 26 || !num_wires || !num_constants)
        return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: null table, no columns or log_n outside 1 .. 26");
    bool needs_pih = false, needs_rc = false, needs_blind = false;
    for (size_t k = 0; k < n_gens; k++) {
        if (!layout_ok(gens[k], num_wires, num_constants))
            return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: a generator's layout leaves the wire table / the constants, or its family is unknown");
        needs_pih |= gens[k].kind == SIPP_GEN_PUBLIC_INPUT;
        needs_rc |= is_poseidon(gens[k].kind);
        needs_blind |= gens[k].kind == SIPP_GEN_RANDOM;
    }
    if (needs_blind && !blind) return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: a Random generator without the blinding seed");
    if (needs_blind) SIPP_TRY(sipp_blind_check(ctx, blind));
    if (needs_pih && !public_inputs_hash) return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: a PublicInput generator without the public-inputs hash");
    SIPP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (needs_rc) {      // the round constants of this translation unit, once per device (a blocking copy: complete before any launch below)
        static std::mutex mu;
        static bool done[64] = {false};
        std::lock_guard<std::mutex> lk(mu);
        const int dev = ctx->device & 63;
        if (!done[dev]) {
            SIPP_CHECK_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(w_rc), SIPP_POSEIDON_RC, sizeof(SIPP_POSEIDON_RC)));
            done[dev] = true;
        }
    }
    return SIPP_OK;
}

extern "C" int sipp_plonk_generate_witness(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, uint32_t num_wires,
                                           uint32_t num_constants, const sipp_plonk_generator* gens, size_t n_gens,
                                           const uint64_t public_inputs_hash[4]) {
    return sipp_plonk_generate_witness_blind(ctx, d_wires, d_constants, log_n, num_wires, num_constants, gens, n_gens, public_inputs_hash, nullptr);
}

// the rows of every SIPP_GEN_RANDOM generator, in front of everything else on the stream (they read no cell)
static int blind_rows_all(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, const sipp_plonk_generator* gens,
                          size_t n_gens, const sipp_blinding* blind) {
    for (size_t k = 0; k < n_gens; k++)
        if (gens[k].kind == SIPP_GEN_RANDOM) SIPP_TRY(sipp_blind_rows_launch(ctx, d_wires, d_constants, log_n, gens[k], *blind));
    return SIPP_OK;
}

extern "C" int sipp_plonk_generate_witness_blind(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n,
                                                 uint32_t num_wires, uint32_t num_constants, const sipp_plonk_generator* gens, size_t n_gens,
                                                 const uint64_t public_inputs_hash[4], const uint64_t* blind_words) {
    if (!ctx) return SIPP_E_BADARG;
    const BlindArg arg(blind_words);
    const sipp_blinding* blind = arg.p;
    SIPP_TRY(witness_prepare(ctx, d_wires, d_constants, log_n, num_wires, num_constants, gens, n_gens, public_inputs_hash, blind));
    SIPP_TRY(blind_rows_all(ctx, d_wires, d_constants, log_n, gens, n_gens, blind));
    const uint32_t n = 1u << log_n;
    for (size_t k = 0; k < n_gens; k++) {
        if (gens[k].kind == SIPP_GEN_RANDOM) continue;
        GenArgs a;
        a.wires = d_wires; a.consts = d_constants; a.n = n; a.g = gens[k];
        for (int l = 0; l < 4; l++) a.pih[l] = public_inputs_hash ? public_inputs_hash[l] : 0;
        ProfScope ps(ctx, gen_name(gens[k].kind));
        if (is_u32_family(gens[k].kind))
            hipLaunchKernelGGL(plonk_witness_u32_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(plonk_witness_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, a);
        SIPP_CHECK_HIP(ctx, hipGetLastError());
    }
    return SIPP_OK;
}

void sipp_witness_graph_release(sipp_ctx* ctx) {
    if (ctx->wgraph.exec) (void)hipGraphExecDestroy(ctx->wgraph.exec);
    if (ctx->wgraph.graph) (void)hipGraphDestroy(ctx->wgraph.graph);
    ctx->wgraph.exec = nullptr;
    ctx->wgraph.graph = nullptr;
    ctx->wgraph.key.clear();
}

namespace {
// the levels of a checked call at one width of the argument struct (Args = LevelArgs or LevelArgsWide)
template <class Args>
int witness_levels_run(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n, uint32_t num_wires, uint32_t num_constants,
                       const sipp_plonk_generator* gens, size_t n_gens, const uint64_t* public_inputs_hash, const sipp_plonk_schedule* sched) {
    const uint32_t n = 1u << log_n, L = sched->n_levels;
    // the error flag lives in a persistent one-word table of the ctx (the captured graph keeps its address)
    int* d_err = reinterpret_cast<int*>(sipp_table_get(ctx, TAB_WITNESS_ERR, 0, 0));
    if (!d_err) {
        uint64_t* t = nullptr;
        SIPP_TRY(sipp_table_put(ctx, TAB_WITNESS_ERR, 0, 0, std::vector<uint64_t>{0}, &t));
        d_err = reinterpret_cast<int*>(t);
    }
    int pos_gen = -1, n_pos = 0;
    bool any_swap = false, any_interp = false, any_initial = false, any_u32 = false;
    for (size_t q = 0; q < n_gens; q++) {
        if (is_poseidon(gens[q].kind)) pos_gen = (int)q, n_pos++;
        any_swap |= gens[q].kind == SIPP_GEN_POSEIDON_SWAP;
        any_interp |= gens[q].kind == SIPP_GEN_COSET_INTERPOLATION;
        any_initial |= gens[q].kind == SIPP_GEN_REDUCING_EXT || gens[q].kind == SIPP_GEN_QUOTIENT_EXT;
        any_u32 |= is_u32_family(gens[q].kind);
    }
    const bool per_row = any_swap || n_pos > 1 || any_interp;     // the lanes go to each row's own Poseidon-family / interpolation generator
    const bool one_lane = any_interp && (ctx->kernel_routes & SIPP_ROUTE_WITNESS_INTERP_ONE_LANE);
    // only a circuit of FRI's initial combination takes the sixteen-lane reduction: every other circuit launches what it always did
    const bool reduce_one_lane = any_initial && (ctx->kernel_routes & SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE);
    // a thin level's per-row kernel at the instantiation the circuit's families need (the one-lane flags are false wherever their code is
    // compiled out); none: the single-generator kernel
    const auto rows_kernel = any_initial  ? (any_u32 ? plonk_witness_level_coop_rows_kernel<true, true, true, Args>
                                                     : plonk_witness_level_coop_rows_kernel<true, true, false, Args>)
                             : any_interp ? (any_u32 ? plonk_witness_level_coop_rows_kernel<true, false, true, Args>
                                                     : plonk_witness_level_coop_rows_kernel<true, false, false, Args>)
                             : per_row    ? (any_u32 ? plonk_witness_level_coop_rows_kernel<false, false, true, Args>
                                                     : plonk_witness_level_coop_rows_kernel<false, false, false, Args>)
                                          : nullptr;
    // a circuit without the u32 and nonnative families launches the instantiations without their code
    const auto level_kernel = any_u32 ? plonk_witness_level_kernel<true, Args> : plonk_witness_level_kernel<false, Args>;
    const auto coop_kernel = any_u32 ? plonk_witness_level_coop_kernel<true, Args> : plonk_witness_level_coop_kernel<false, Args>;
    Args a;          // the same for every level but for rows and count
    a.wires = d_wires; a.consts = d_constants; a.n = n; a.n_gens = (uint32_t)n_gens; a.err = d_err;
    for (int q = 0; q < 4; q++) a.pih[q] = public_inputs_hash ? public_inputs_hash[q] : 0;
    for (size_t q = 0; q < n_gens; q++) a.g[q] = gens[q];
    auto launch_all = [&]() -> hipError_t {
        (void)hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream);
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t r0 = sched->level_offsets[l], cnt = sched->level_offsets[l + 1] - r0;
            if (cnt) {
                a.rows = sched->d_rows + r0;
                a.count = cnt;
                if (cnt >= COOP_BELOW_ROWS)      // wide level: throughput, one lane per row
                    hipLaunchKernelGGL(level_kernel, dim3((cnt + 63) / 64), dim3(64), 0, ctx->stream, a);
                else if (rows_kernel)            // thin level: latency, sixteen lanes per row
                    hipLaunchKernelGGL(rows_kernel, dim3((cnt + 3) / 4), dim3(64), 0, ctx->stream, a, one_lane, reduce_one_lane);
                else
                    hipLaunchKernelGGL(coop_kernel, dim3((cnt + 3) / 4), dim3(64), 0, ctx->stream, a, pos_gen);
            }
            const uint32_t c0 = sched->copy_offsets[l], cc = sched->copy_offsets[l + 1] - c0;
            if (cc)
                hipLaunchKernelGGL(plonk_witness_copy_kernel, dim3((cc + 255) / 256), dim3(256), 0, ctx->stream, d_wires, sched->d_copy_src + c0,
                                   sched->d_copy_dst + c0, cc, (uint64_t)num_wires << log_n, d_err);
        }
        return hipGetLastError();
    };
    const bool use_graph = !ctx->prof && !(ctx->kernel_routes & SIPP_ROUTE_WITNESS_NO_GRAPH);
    if (!use_graph) {
        ProfScope ps(ctx, "witness_levels");
        SIPP_CHECK_HIP(ctx, launch_all());
    } else {
        // key: everything the captured kernel arguments hold
        std::vector<uint64_t> key = {(uint64_t)(uintptr_t)d_wires, (uint64_t)(uintptr_t)d_constants, log_n, num_wires, num_constants, n_gens, L,
                                     (uint64_t)one_lane | ((uint64_t)reduce_one_lane << 1),
                                     (uint64_t)(uintptr_t)sched->d_rows, (uint64_t)(uintptr_t)sched->d_copy_src, (uint64_t)(uintptr_t)sched->d_copy_dst};
        for (int q = 0; q < 4; q++) key.push_back(public_inputs_hash ? public_inputs_hash[q] : 0);
        for (size_t q = 0; q < n_gens; q++) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(&gens[q]);
            for (size_t x = 0; x < sizeof(sipp_plonk_generator) / 4; x++) key.push_back(w[x]);
        }
        for (uint32_t l = 0; l <= L; l++) key.push_back(((uint64_t)sched->level_offsets[l] << 32) | sched->copy_offsets[l]);
        if (!ctx->wgraph.exec || ctx->wgraph.key != key) {
            sipp_witness_graph_release(ctx);
            SIPP_CHECK_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
            const hipError_t le = launch_all();
            hipGraph_t g = nullptr;
            const hipError_t ce = hipStreamEndCapture(ctx->stream, &g);
            if (le != hipSuccess || ce != hipSuccess || !g) {
                if (g) (void)hipGraphDestroy(g);
                return sipp_fail(ctx, SIPP_E_HIP, "plonk witness: capturing the level launches as a hipGraph failed");
            }
            ctx->wgraph.graph = g;
            if (hipGraphInstantiate(&ctx->wgraph.exec, g, nullptr, nullptr, 0) != hipSuccess) {
                sipp_witness_graph_release(ctx);
                return sipp_fail(ctx, SIPP_E_HIP, "plonk witness: hipGraphInstantiate failed");
            }
            ctx->wgraph.key = key;
        }
        SIPP_CHECK_HIP(ctx, hipGraphLaunch(ctx->wgraph.exec, ctx->stream));
    }
    int h_err = 0;
    SIPP_CHECK_HIP(ctx, hipMemcpyAsync(&h_err, d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SIPP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_err) return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: the schedule names a row or a cell outside the wire table");
    return SIPP_OK;
}
}  // namespace

extern "C" int sipp_plonk_generate_witness_levels(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n,
                                                  uint32_t num_wires, uint32_t num_constants, const sipp_plonk_generator* gens, size_t n_gens,
                                                  const uint64_t public_inputs_hash[4], const sipp_plonk_schedule* sched) {
    return sipp_plonk_generate_witness_levels_blind(ctx, d_wires, d_constants, log_n, num_wires, num_constants, gens, n_gens, public_inputs_hash,
                                                    sched, nullptr);
}

extern "C" int sipp_plonk_generate_witness_levels_blind(sipp_ctx* ctx, uint64_t* d_wires, const uint64_t* d_constants, uint32_t log_n,
                                                        uint32_t num_wires, uint32_t num_constants, const sipp_plonk_generator* gens,
                                                        size_t n_gens, const uint64_t public_inputs_hash[4], const sipp_plonk_schedule* sched,
                                                        const uint64_t* blind_words) {
    if (!ctx) return SIPP_E_BADARG;
    const BlindArg arg(blind_words);
    const sipp_blinding* blind = arg.p;
    // the ceiling first: nothing is launched, copied or uploaded for a circuit past it
    if (n_gens > MAX_GENS) return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: more than 32 generators (the level kernels carry at most 32)");
    SIPP_TRY(witness_prepare(ctx, d_wires, d_constants, log_n, num_wires, num_constants, gens, n_gens, public_inputs_hash, blind));
    if (!sched || !sched->n_levels || sched->n_levels > (1u << 20) || !sched->d_rows || !sched->level_offsets || !sched->copy_offsets)
        return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: no schedule or no level");
    const uint32_t n = 1u << log_n, L = sched->n_levels;
    for (uint32_t l = 0; l < L; l++)
        if (sched->level_offsets[l] > sched->level_offsets[l + 1] || sched->copy_offsets[l] > sched->copy_offsets[l + 1])
            return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: schedule offsets must not decrease");
    if (sched->level_offsets[L] > n || (sched->copy_offsets[L] && (!sched->d_copy_src || !sched->d_copy_dst)))
        return sipp_fail(ctx, SIPP_E_BADARG, "plonk witness: more scheduled rows than the table has, or copies without their cell lists");
    // blinding rows first, outside the captured graph (the seed and counter change from proof to proof, the graph's arguments do not)
    SIPP_TRY(blind_rows_all(ctx, d_wires, d_constants, log_n, gens, n_gens, blind));
    // a circuit at or below NARROW_GENS launches the kernels, with the arguments, it launched before the ceiling rose
    return n_gens <= NARROW_GENS
               ? witness_levels_run<LevelArgs>(ctx, d_wires, d_constants, log_n, num_wires, num_constants, gens, n_gens, public_inputs_hash, sched)
               : witness_levels_run<LevelArgsWide>(ctx, d_wires, d_constants, log_n, num_wires, num_constants, gens, n_gens, public_inputs_hash, sched);
}
