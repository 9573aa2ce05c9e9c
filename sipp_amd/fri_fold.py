"""FRI fold chains in the outer circuit: plonky2's ArithmeticExtensionGate, ExponentiationGate and CosetInterpolationGate as gate programs,
and a circuit that proves what fri_verifier_query_round does for every query after the Merkle paths (fri/recursive_verifier.rs, recalled).

  arithmetic_ext_gate       2 constraints per op:  output - (c0 a b + c1 c)  over F[X]/(X^2 - W), limb by limb
  exponentiation_gate       n_bits + 1 constraints:  prev^2 (bit base + 1 - bit) - intermediate_i,  output - last intermediate
  coset_interpolation_gate  shifted shift - point; per chunk the computed (eval, product) minus their wires; the last eval minus the
                            evaluation value -- every constraint expanded into base-field monomials, the domain points x_i = g^i and the
                            barycentric weights w_i = g^i / n folded into the coefficients
  FriFoldCircuit            the gate set, the rows, the copy cycles (sigmas), the generators and the level schedule of the statement
                            "every query's fold chain leads from its first value to the final polynomial"
  FriFoldProver             the circuit through the library's CircuitData: built once, then prove(fold data) / verify

Layouts are the generators' (include/sipp_hip.h, SIPP_GEN_ARITHMETIC_EXT / _EXPONENTIATION / _COSET_INTERPOLATION).

Statement layout.  Public inputs = beta_r (ext) per round || the final polynomial (ext coefficients) || per query (x_index, the value `old`
entering the first fold (ext), the 2^arity_bits ext evals of every round).  They are hashed in circuit by the swap-0 Poseidon chain and
tied to the PublicInput gate as in sipp_amd/merkle.py.  Per query: a BaseSum row (1-bit limbs) splits x_index; an Exponentiation row raises
omega_M to rev(x_index) (its bit wires are the limbs in reverse order); an arithmetic op multiplies by the coset generator 7: x.  Per round:
two RandomAccess copies check evals[within] = old limb by limb (their bit wires are the low limbs of the current index bits); an
Exponentiation row gives (g^-1)^rev(within), an arithmetic op multiplies it by x: the shift; a CosetInterpolation row takes the evals in
bit-reversed order and beta_r, its evaluation value is the next `old`; arity_bits squarings of x; the index drops its low arity_bits bits.
ArithmeticExt rows then evaluate the final polynomial at (x, 0) by Horner; the result is the last `old`.

Out of scope: fri_combine_initial (the first `old` is a public input; sipp_amd/fri_initial.py proves it); the Merkle paths of the opened cosets (MerkleOpeningCircuit's job);
the proof of work; mixed arities (one arity for every round: plonky2's ConstantArityBits).

numpy only; imports nothing from the test oracle."""
import numpy as np

from .merkle import (GEN_BASE_SPLIT, GEN_CONSTANT, GEN_POSEIDON_SWAP, GEN_PUBLIC_INPUT, GEN_RANDOM_ACCESS, P, SWAP_LAYOUT, UNUSED, _K, _PIH,
                     _Prog, _W, _gl_mul, _powers, _root_of_unity, _swap_gate_into, fri_params)

# include/sipp_hip.h SIPP_GEN_*
GEN_ARITHMETIC_EXT, GEN_EXPONENTIATION, GEN_COSET_INTERPOLATION = 10, 11, 12
EXT_W = 7                                       # X^2 = 7
COSET_GEN = 7                                   # the LDE coset's shift
MAX_MONOMIALS, MAX_FACTORS = 4096, 64           # the constraint interpreter's limits
GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "ArithmeticExt", "RandomAccess", "Exponentiation", "PoseidonSwap", "CosetInterpolation"]
NOOP, PUBLIC_INPUT, CONSTANT, BASE_SUM, ARITHMETIC_EXT, RANDOM_ACCESS, EXPONENTIATION, POSEIDON_SWAP, COSET_INTERPOLATION = range(9)
# selector groups [lo, hi): filter degree (hi - lo - 1) + 1, and with the gate's degree at most 8
GROUPS = ((0, 5), (5, 7), (7, 8), (8, 9))
_C0, _C1 = 4, 5                                 # the two constant columns behind the four selector columns
INTERP_DEGREE = 7                               # alone in its group: filter degree 1


def reverse_bits(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


# ---- polynomials over the wires: {sorted tuple of wire indices: coefficient} --------------------------------------------------------------
def _padd(a, b, sb=1):
    r = dict(a)
    for k, v in b.items():
        r[k] = (r.get(k, 0) + sb * v) % P
    return r


def _pmul(a, b):
    r = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            k = tuple(sorted(ka + kb))
            r[k] = (r.get(k, 0) + va * vb) % P
    return r


def _pscale(a, s):
    return {k: v * s % P for k, v in a.items()}


def _emul(x, y, W):
    return (_padd(_pmul(x[0], y[0]), _pscale(_pmul(x[1], y[1]), W)), _padd(_pmul(x[0], y[1]), _pmul(x[1], y[0])))


def _wire(w):
    return {(w,): 1}


def _emit(pr, poly):
    monos = [(c, [(_W, w) for w in k]) for k, c in poly.items() if c]
    assert len(monos) <= MAX_MONOMIALS and max([len(f) for _, f in monos] or [0]) <= MAX_FACTORS
    pr.constraint(monos)


def interpolation_layout(s, d):
    """wire positions of SIPP_GEN_COSET_INTERPOLATION: n points, ni intermediates"""
    n = 1 << s
    ni = (n - 2) // (d - 1)
    start = 5 + 2 * n
    return {"n": n, "ni": ni, "shift": 0, "values": 1, "point": 1 + 2 * n, "eval": 3 + 2 * n, "ie": start, "ip": start + 2 * ni,
            "shifted": start + 4 * ni, "num_wires": start + 4 * ni + 2}


def _arithmetic_ext_into(pr, n_ops, c0, c1, W):
    for k in range(n_ops):
        b = 8 * k
        a0, a1, m0, m1 = (_W, b), (_W, b + 1), (_W, b + 2), (_W, b + 3)
        for monos in ([(1, [(_W, b + 6)]), (-1, [(_K, c0), a0, m0]), (-W, [(_K, c0), a1, m1]), (-1, [(_K, c1), (_W, b + 4)])],
                      [(1, [(_W, b + 7)]), (-1, [(_K, c0), a0, m1]), (-1, [(_K, c0), a1, m0]), (-1, [(_K, c1), (_W, b + 5)])]):
            pr.constraint(monos)


def _exponentiation_into(pr, n_bits):
    base = (_W, 0)
    for i in range(n_bits):
        bit, inter = (_W, n_bits - i), (_W, 2 + n_bits + i)
        sq = [(_W, 1 + n_bits + i)] * 2 if i else []                     # prev^2; prev_0 = 1
        pr.constraint([(1, sq + [bit, base]), (1, sq), (-1, sq + [bit]), (-1, [inter])])
    pr.constraint([(1, [(_W, 1 + n_bits)]), (-1, [(_W, 1 + 2 * n_bits)])])


def _coset_interpolation_into(pr, s, d, W):
    lay = interpolation_layout(s, d)
    n, ni = lay["n"], lay["ni"]
    g, ninv = _root_of_unity(s), pow(n, P - 2, P)
    sh = (_wire(lay["shifted"]), _wire(lay["shifted"] + 1))
    for l in range(2):                                                    # shifted shift - point
        _emit(pr, _padd(_pmul(sh[l], _wire(lay["shift"])), _wire(lay["point"] + l), -1))
    e, q = ({}, {}), ({(): 1}, {})
    bound, c = min(d, n), 0
    for i in range(n):
        x = pow(g, i, P)
        wt = x * ninv % P
        t = (_padd(sh[0], {(): x}, -1), sh[1])
        vw = (_pscale(_wire(lay["values"] + 2 * i), wt), _pscale(_wire(lay["values"] + 2 * i + 1), wt))
        et, vq = _emul(e, t, W), _emul(vw, q, W)
        e, q = (_padd(et[0], vq[0]), _padd(et[1], vq[1])), _emul(q, t, W)
        if i + 1 == bound and i + 1 < n:
            for l in range(2):
                _emit(pr, _padd(e[l], _wire(lay["ie"] + 2 * c + l), -1))
            for l in range(2):
                _emit(pr, _padd(q[l], _wire(lay["ip"] + 2 * c + l), -1))
            e = (_wire(lay["ie"] + 2 * c), _wire(lay["ie"] + 2 * c + 1))
            q = (_wire(lay["ip"] + 2 * c), _wire(lay["ip"] + 2 * c + 1))
            c += 1
            bound += d - 1
    assert c == ni
    for l in range(2):
        _emit(pr, _padd(e[l], _wire(lay["eval"] + l), -1))


def _words(fill, *args):
    pr = _Prog()
    fill(pr, *args)
    return pr, np.array(pr.words, dtype=np.int64)


def arithmetic_ext_gate(n_ops, c0, c1, W=EXT_W):
    """ArithmeticExtensionGate: per op at b = 8k the two limbs of  output - (const[c0] a b + const[c1] c);  degree 3"""
    assert n_ops >= 1 and W % P
    pr, words = _words(_arithmetic_ext_into, n_ops, c0, c1, W)
    assert pr.count == 2 * n_ops
    return words


def exponentiation_gate(n_bits):
    """ExponentiationGate: prev^2 (bit base + 1 - bit) - intermediate_i for the bits from the top wire down (prev_0 = 1), then
    output - last intermediate; no booleanity (upstream's gate has none); degree 4"""
    assert 1 <= n_bits <= 64
    pr, words = _words(_exponentiation_into, n_bits)
    assert pr.count == n_bits + 1
    return words


def coset_interpolation_gate(s, d, W=EXT_W):
    """CosetInterpolationGate over the subgroup of order 2^s with chunks of degree d: 2 + 4 ni + 2 constraints, degree min(d, 2^s)"""
    assert 1 <= s <= 4 and d >= 2 and W % P
    pr, words = _words(_coset_interpolation_into, s, d, W)
    assert pr.count == 4 + 4 * interpolation_layout(s, d)["ni"]
    return words


class _Cells:
    """union-find over cells: every set of tied cells becomes one permutation cycle"""

    def __init__(self):
        self.parent = {}

    def find(self, x):
        p = self.parent.setdefault(x, x)
        while p != self.parent[p]:
            self.parent[p] = self.parent[self.parent[p]]
            p = self.parent[p]
        self.parent[x] = p
        return p

    def tie(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            self.parent[max(ra, rb)] = min(ra, rb)

    def groups(self):
        out = {}
        for x in sorted(self.parent):
            out.setdefault(self.find(x), []).append(x)
        return out


class FriFoldCircuit:
    """The circuit of the fold chains of n_queries queries of a FRI opening proof over an LDE of 2^log_m points: n_rounds rounds of arity
    2^arity_bits, a final polynomial of final_len ext coefficients.  Cells are wire * N + row."""

    def __init__(self, log_m, arity_bits, n_rounds, final_len, n_queries, num_wires=135, num_routed=80, min_log_n=10):
        assert 1 <= arity_bits <= 4 and n_rounds >= 1 and arity_bits * n_rounds <= log_m <= 64 and final_len >= 1 and n_queries >= 1
        assert 2 + 2 * log_m <= num_wires and 2 + log_m <= num_routed and num_wires >= 135
        self.log_m, self.arity_bits, self.n_rounds, self.final_len, self.n_queries = log_m, arity_bits, n_rounds, final_len, n_queries
        self.num_wires, self.num_routed = num_wires, num_routed
        self.arity = 1 << arity_bits
        lay = SWAP_LAYOUT
        self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox = lay["in_"], lay["out"], lay["swap"], lay["delta"], lay["sbox"]
        self.ra_stride = 2 + self.arity + arity_bits
        assert self.ra_stride + 2 + self.arity + arity_bits <= num_routed
        self.interp = interpolation_layout(arity_bits, INTERP_DEGREE)
        assert self.interp["point"] + 4 <= num_routed and self.interp["num_wires"] <= num_wires
        self.omega_m = _root_of_unity(log_m)
        self.g_inv = pow(_root_of_unity(arity_bits), P - 2, P)
        self.n_pi = 2 * n_rounds + 2 * final_len + n_queries * (3 + 2 * self.arity * n_rounds)
        self.n_pi_rows = -(-self.n_pi // 8)
        self._layout_rows(min_log_n)
        self._programs()
        self._wiring()

    # public-input positions
    def pi_beta(self, r, l):
        return 2 * r + l

    def pi_final(self, k, l):
        return 2 * self.n_rounds + 2 * k + l

    def pi_query(self, q):
        return 2 * self.n_rounds + 2 * self.final_len + q * (3 + 2 * self.arity * self.n_rounds)

    def pi_eval(self, q, r, j, l):
        return self.pi_query(q) + 3 + 2 * (self.arity * r + j) + l

    # ---- rows ----
    def _layout_rows(self, min_log_n):
        self.pi_row, self.zero_row, self.omega_row, self.ginv_row = 0, 1, 2, 3
        r = 4
        R, a = self.n_rounds, self.arity_bits
        self.bs_row, self.exp0_row, self.x_row, self.ra_row, self.exp_row, self.shift_row, self.interp_row, self.sq_row, self.horner_row = (
            [], [], [], [], [], [], [], [], [])
        for _ in range(self.n_queries):
            self.bs_row.append(r); self.exp0_row.append(r + 1); self.x_row.append(r + 2)
            r += 3
            ra, ex, sf, it, sq = [], [], [], [], []
            for _r in range(R):
                ra.append(r); ex.append(r + 1); sf.append(r + 2); it.append(r + 3)
                sq.append(list(range(r + 4, r + 4 + a)))
                r += 4 + a
            self.ra_row.append(ra); self.exp_row.append(ex); self.shift_row.append(sf); self.interp_row.append(it); self.sq_row.append(sq)
            self.horner_row.append(list(range(r, r + self.final_len - 1)))
            r += self.final_len - 1
        self.chain_row = list(range(r, r + self.n_pi_rows))
        r += self.n_pi_rows
        self.rows_used = r
        self.log_n = max(min_log_n, (r - 1).bit_length())
        self.n = 1 << self.log_n
        gate = np.full(self.n, NOOP, dtype=np.int64)
        c0 = np.zeros(self.n, dtype=np.uint64)
        c1 = np.zeros(self.n, dtype=np.uint64)
        gate[self.pi_row] = PUBLIC_INPUT
        gate[[self.zero_row, self.omega_row, self.ginv_row]] = CONSTANT
        c0[self.omega_row], c0[self.ginv_row] = self.omega_m, self.g_inv
        for q in range(self.n_queries):
            gate[self.bs_row[q]] = BASE_SUM
            gate[[self.exp0_row[q]] + self.exp_row[q]] = EXPONENTIATION
            gate[self.ra_row[q]] = RANDOM_ACCESS
            gate[self.interp_row[q]] = COSET_INTERPOLATION
            mul = self.shift_row[q] + [x for s in self.sq_row[q] for x in s]
            gate[[self.x_row[q]] + mul + self.horner_row[q]] = ARITHMETIC_EXT
            c1[self.x_row[q]] = COSET_GEN                                    # 0 a b + 7 c
            c0[mul] = 1                                                      # a b
            c0[self.horner_row[q]] = 1                                       # a b + c
            c1[self.horner_row[q]] = 1
        gate[self.chain_row] = POSEIDON_SWAP
        self.gate, self.c0, self.c1 = gate, c0, c1

    def _programs(self):
        pr, gates = _Prog(), []

        def add(index, group, fill):
            off, cnt = len(pr.words), pr.count
            fill()
            gates.append((group, index, GROUPS[group][0], GROUPS[group][1], off, pr.count - cnt))
        add(NOOP, 0, lambda: None)
        add(PUBLIC_INPUT, 0, lambda: [pr.constraint([(1, [(_W, i)]), (-1, [(_PIH, i)])]) for i in range(4)])
        add(CONSTANT, 0, lambda: pr.constraint([(1, [(_W, 0)]), (-1, [(_K, _C0)])]))

        def base_sum():
            pr.constraint([(1 << i, [(_W, 1 + i)]) for i in range(self.log_m)] + [(-1, [(_W, 0)])])
            for i in range(self.log_m):
                pr.constraint([(1, [(_W, 1 + i), (_W, 1 + i)]), (-1, [(_W, 1 + i)])])
        add(BASE_SUM, 0, base_sum)
        add(ARITHMETIC_EXT, 0, lambda: _arithmetic_ext_into(pr, 1, _C0, _C1, EXT_W))

        def random_access():
            ab, ln = self.arity_bits, self.arity
            for cp in range(2):
                b = self.ra_stride * cp
                bits = [(_W, b + 2 + ln + l) for l in range(ab)]
                for x in bits:
                    pr.constraint([(1, [x, x]), (-1, [x])])
                pr.constraint([(1 << l, [bits[l]]) for l in range(ab)] + [(-1, [(_W, b)])])
                monos = []
                for j in range(ln):
                    terms = [(1, [(_W, b + 2 + j)])]
                    for l in range(ab):
                        if (j >> l) & 1:
                            terms = [(c, f + [bits[l]]) for c, f in terms]
                        else:
                            terms = [t for c, f in terms for t in ((c, f), (-c, f + [bits[l]]))]
                    monos += terms
                pr.constraint(monos + [(-1, [(_W, b + 1)])])
        add(RANDOM_ACCESS, 1, random_access)
        add(EXPONENTIATION, 1, lambda: _exponentiation_into(pr, self.log_m))
        add(POSEIDON_SWAP, 2, lambda: _swap_gate_into(pr, self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox))
        add(COSET_INTERPOLATION, 3, lambda: _coset_interpolation_into(pr, self.arity_bits, INTERP_DEGREE, EXT_W))
        self.gates, self.programs = gates, np.array(pr.words, dtype=np.int64)
        self.gate_degree = [0, 1, 1, 2, 3, self.arity_bits + 1, 4, 7, min(INTERP_DEGREE, self.arity)]
        for (grp, idx, lo, hi, _, _), deg in zip(gates, self.gate_degree):
            assert (hi - lo - 1) + 1 + deg <= 8, GATE_NAMES[idx]

    # ---- copy cycles and the level schedule ----
    def _wiring(self):
        n, R, a, A, M = self.n, self.n_rounds, self.arity_bits, self.arity, self.log_m
        cell = lambda w, r: w * n + r
        uf = _Cells()
        copies = []                                     # (level of the source, src cell, dst cell)
        row_level = np.full(n, -1, dtype=np.int64)
        zero = cell(0, self.zero_row)
        self.pi_cells = [None] * self.n_pi              # one cell of public input t: every cell of its cycle takes its value
        self.input_cells = []                           # per query per round the RandomAccess index cells (partial witness: `within`)

        def copy(level, src, dst):
            uf.tie(src, dst)
            copies.append((level, src, dst))

        def pi(t, c):
            if self.pi_cells[t] is None:
                self.pi_cells[t] = c
            uf.tie(self.pi_cells[t], c)
        row_level[[self.pi_row, self.zero_row, self.omega_row, self.ginv_row]] = 0
        # the PI chain: row j absorbs pis[8 j .. 8 j + len_j)
        for j, r in enumerate(self.chain_row):
            row_level[r] = 1 + j
            ln = min(8, self.n_pi - 8 * j)
            for t in range(ln):
                pi(8 * j + t, cell(self.s_in + t, r))
            for t in range(ln, 12):
                if j == 0:
                    copy(0, zero, cell(self.s_in + t, r))
                else:
                    copy(j, cell(self.s_out + t, self.chain_row[j - 1]), cell(self.s_in + t, r))
            copy(0, zero, cell(self.s_swap, r))
        for t in range(4):
            uf.tie(cell(self.s_out + t, self.chain_row[-1]), cell(t, self.pi_row))
        it = self.interp
        last_level = 0
        for q in range(self.n_queries):
            base = self.pi_query(q)
            bs, e0, xr = self.bs_row[q], self.exp0_row[q], self.x_row[q]
            row_level[bs], row_level[e0], row_level[xr] = 0, 1, 2
            pi(base, cell(0, bs))
            bits = [cell(1 + i, bs) for i in range(M)]                       # the current index bits, low first
            # omega_M ^ rev(x_index): exponent bit j = index bit M - 1 - j
            copy(0, cell(0, self.omega_row), cell(0, e0))
            for j in range(M):
                copy(0, bits[M - 1 - j], cell(1 + j, e0))
            # x = 7 (omega_M ^ rev, 0): the c operand
            copy(1, cell(1 + M, e0), cell(4, xr))
            copy(0, zero, cell(5, xr))
            x, x_level = cell(6, xr), 2
            old = [None, None]
            for l in range(2):
                pi(base + 1 + l, cell(1 + self.ra_stride * l, self.ra_row[q][0]))      # the first old = the claimed element of round 0
                old[l] = self.pi_cells[base + 1 + l]
            inputs = []
            for r in range(R):
                ra, ex, sf, ir = self.ra_row[q][r], self.exp_row[q][r], self.shift_row[q][r], self.interp_row[q][r]
                row_level[ra], row_level[ex] = 0, 1
                idx_cells = []
                for l in range(2):                                               # evals[within] = old, limb l
                    b = self.ra_stride * l
                    idx_cells.append(cell(b, ra))
                    uf.tie(old[l], cell(b + 1, ra))
                    for j in range(A):
                        pi(self.pi_eval(q, r, j, l), cell(b + 2 + j, ra))
                    for t in range(a):
                        uf.tie(bits[t], cell(b + 2 + A + t, ra))
                inputs.append(idx_cells)
                # (g^-1) ^ rev(within): exponent bit j = index bit a - 1 - j, the bits above are 0
                copy(0, cell(0, self.ginv_row), cell(0, ex))
                for j in range(M):
                    copy(0, bits[a - 1 - j] if j < a else zero, cell(1 + j, ex))
                # shift = (g^-1)^rev x
                row_level[sf] = x_level + 1
                copy(1, cell(1 + M, ex), cell(0, sf))
                copy(x_level, x, cell(2, sf))
                copy(0, zero, cell(1, sf))
                copy(0, zero, cell(3, sf))
                # the interpolation at beta_r of the evals in bit-reversed order
                row_level[ir] = x_level + 2
                copy(x_level + 1, cell(6, sf), cell(it["shift"], ir))
                for k in range(A):
                    for l in range(2):
                        pi(self.pi_eval(q, r, reverse_bits(k, a), l), cell(it["values"] + 2 * k + l, ir))
                for l in range(2):
                    pi(self.pi_beta(r, l), cell(it["point"] + l, ir))
                old = [cell(it["eval"], ir), cell(it["eval"] + 1, ir)]
                last_level = max(last_level, x_level + 2)
                # x <- x^arity
                for sq in self.sq_row[q][r]:
                    row_level[sq] = x_level + 1
                    copy(x_level, x, cell(0, sq))
                    copy(x_level, x, cell(2, sq))
                    copy(0, zero, cell(1, sq))
                    copy(0, zero, cell(3, sq))
                    x, x_level = cell(6, sq), x_level + 1
                bits = bits[a:]
            self.input_cells.append(inputs)
            # the final polynomial at (x, 0) by Horner: acc = c_(F-1); acc <- acc (x, 0) + c_k
            F = self.final_len
            acc = [self.pi_cells[self.pi_final(F - 1, l)] for l in range(2)]
            acc_level = None
            for step, hr in enumerate(self.horner_row[q]):
                k = F - 2 - step
                row_level[hr] = x_level + 1 + step
                for l in range(2):
                    if acc_level is None:
                        pi(self.pi_final(F - 1, l), cell(l, hr))
                    else:
                        copy(acc_level, acc[l], cell(l, hr))
                    pi(self.pi_final(k, l), cell(4 + l, hr))
                copy(x_level, x, cell(2, hr))
                copy(0, zero, cell(3, hr))
                acc, acc_level = [cell(6, hr), cell(7, hr)], x_level + 1 + step
                last_level = max(last_level, acc_level)
            for l in range(2):
                if acc[l] is None:                                               # F = 1 and the coefficient has no cell yet
                    pi(self.pi_final(0, l), old[l])
                else:
                    uf.tie(acc[l], old[l])
        groups = uf.groups()
        self.cycles = [g for g in groups.values() if len(g) > 1]
        self.pi_cycle = [groups[uf.find(c)] for c in self.pi_cells]
        self.row_level = row_level
        self.n_levels = int(row_level.max()) + 1
        lev = np.array([c[0] for c in copies], dtype=np.int64)
        src = np.array([c[1] for c in copies], dtype=np.uint64)
        dst = np.array([c[2] for c in copies], dtype=np.uint64)
        o = np.argsort(lev, kind="stable")
        lev, src, dst = lev[o], src[o], dst[o]
        sched_rows = np.flatnonzero(row_level >= 0)
        rows = sched_rows[np.lexsort((sched_rows, self.gate[sched_rows], row_level[sched_rows]))].astype(np.uint32)
        self._schedule = {"n_levels": self.n_levels, "row_level": row_level, "rows": rows,
                          "level_offsets": np.searchsorted(row_level[rows], np.arange(self.n_levels + 1)).astype(np.uint32),
                          "copy_src": src, "copy_dst": dst,
                          "copy_offsets": np.searchsorted(lev, np.arange(self.n_levels + 1)).astype(np.uint32)}

    # ---- the public face ----
    def circuit(self):
        """the circuit dict of tools/plonk_synth.circuit(): num_wires, num_routed, num_constants, num_selectors, gates, programs"""
        return {"num_wires": self.num_wires, "num_routed": self.num_routed, "num_constants": 6, "num_selectors": 4, "gates": list(self.gates),
                "programs": self.programs, "num_gate_constraints": max(g[5] for g in self.gates), "gate_names": GATE_NAMES}

    def generators(self):
        """[(kind, selector_index, row, p0 .. p4)] (include/sipp_hip.h sipp_plonk_generator)"""
        return [(GEN_PUBLIC_INPUT, 0, PUBLIC_INPUT, 0, 0, 0, 0, 0),
                (GEN_CONSTANT, 0, CONSTANT, 1, _C0, 0, 0, 0),
                (GEN_BASE_SPLIT, 0, BASE_SUM, self.log_m, 1, 0, 0, 0),
                (GEN_ARITHMETIC_EXT, 0, ARITHMETIC_EXT, 1, _C0, _C1, EXT_W, 0),
                (GEN_RANDOM_ACCESS, 1, RANDOM_ACCESS, 2, self.ra_stride, self.arity_bits, 0, 0),
                (GEN_EXPONENTIATION, 1, EXPONENTIATION, self.log_m, 0, 0, 0, 0),
                (GEN_POSEIDON_SWAP, 2, POSEIDON_SWAP, self.s_in, self.s_out, self.s_sbox, self.s_swap, self.s_delta),
                (GEN_COSET_INTERPOLATION, 3, COSET_INTERPOLATION, self.arity_bits, INTERP_DEGREE, EXT_W, 0, 0)]

    def schedule(self):
        """the level schedule of sipp_plonk_generate_witness_levels"""
        return self._schedule

    def constants_sigmas(self):
        """[6 + num_routed][N]: the four selector columns, the two constant columns, the sigmas of the copy cycles (k_i = 7^i)"""
        n, R = self.n, self.num_routed
        sels = [np.where((self.gate >= lo) & (self.gate < hi), self.gate, UNUSED).astype(np.uint64) for lo, hi in GROUPS]
        perm = np.arange(R * n, dtype=np.int64)
        for cyc in self.cycles:
            c = np.asarray(cyc, dtype=np.int64)
            assert int(c.max()) < R * n
            perm[c] = np.roll(c, -1)
        pw = _powers(_root_of_unity(self.log_n), n)
        ks = np.array([pow(7, j, P) for j in range(R)], dtype=np.uint64)
        pm = perm.reshape(R, n)
        sig = np.empty((R, n), dtype=np.uint64)
        for j in range(R):
            sig[j] = _gl_mul(ks[pm[j] >> self.log_n], pw[pm[j] & (n - 1)])
        return np.ascontiguousarray(np.concatenate([np.stack(sels + [self.c0, self.c1]), sig]).astype(np.uint64))

    def _check(self, betas, final_poly, queries):
        betas = [(int(b[0]) % P, int(b[1]) % P) for b in betas]
        final_poly = [(int(c[0]) % P, int(c[1]) % P) for c in final_poly]
        assert len(betas) == self.n_rounds and len(final_poly) == self.final_len and len(queries) == self.n_queries
        out = []
        for x_index, old, evals in queries:
            x_index = int(x_index)
            assert 0 <= x_index < (1 << self.log_m) and len(evals) == self.n_rounds
            ev = [[(int(v[0]) % P, int(v[1]) % P) for v in rnd] for rnd in evals]
            assert all(len(rnd) == self.arity for rnd in ev)
            out.append((x_index, (int(old[0]) % P, int(old[1]) % P), ev))
        return betas, final_poly, out

    def public_inputs(self, betas, final_poly, queries):
        """betas || final polynomial || per query (x_index, old, evals of every round), as ints; ext values as (c0, c1) pairs"""
        betas, final_poly, queries = self._check(betas, final_poly, queries)
        out = [l for b in betas for l in b] + [l for c in final_poly for l in c]
        for x_index, old, evals in queries:
            out += [x_index, old[0], old[1]] + [l for rnd in evals for v in rnd for l in v]
        assert len(out) == self.n_pi
        return out

    def partial_witness(self, betas, final_poly, queries):
        """[num_wires][N] with the INPUT cells set: every cell on a cycle of a public input, and the RandomAccess indices (the index
        within the coset of every round); everything else 0"""
        pis = self.public_inputs(betas, final_poly, queries)
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        flat = w.reshape(-1)
        for t, cyc in enumerate(self.pi_cycle):
            flat[np.asarray(cyc, dtype=np.int64)] = np.uint64(pis[t])
        for q, (x_index, _, _) in enumerate(self._check(betas, final_poly, queries)[2]):
            for r in range(self.n_rounds):
                within = (x_index >> (self.arity_bits * r)) & (self.arity - 1)
                flat[np.asarray(self.input_cells[q][r], dtype=np.int64)] = np.uint64(within)
        return w


class FriFoldProver:
    """FriFoldCircuit through the library's CircuitData: the constants_sigmas commitment and the schedule go to the device once;
    prove(betas, final_poly, queries) generates the witness there and returns the flat proof."""

    def __init__(self, ctx, log_m, arity_bits, n_rounds, final_len, n_queries, fri=None, params=None, digest=None, min_log_n=10):
        from . import _lib
        self.circ = FriFoldCircuit(log_m, arity_bits, n_rounds, final_len, n_queries, min_log_n=min_log_n)
        c = self.circ
        self.params = params if params is not None else _lib.PlonkParams(c.num_routed, 8, 2)
        self.fri = fri if fri is not None else fri_params(c.log_n)
        self.circuit = self.circ.circuit()
        self._pc = _lib.PlonkCircuit.from_dict(self.circuit)
        self.data = _lib.CircuitData(ctx, c.log_n, self.params, self.fri, self._pc, c.constants_sigmas(), c.generators(), sched=c.schedule(),
                                     digest=digest)
        self.cap, self.digest = self.data.cap, self.data.digest

    def prove(self, betas, final_poly, queries):
        c = self.circ
        return self.data.prove(c.partial_witness(betas, final_poly, queries), c.public_inputs(betas, final_poly, queries))

    def verify(self, proof):
        """-> (status, refusing stage): (0, 0) = accepted"""
        return self.data.verify(proof)

    def close(self):
        self.data.close()
