"""FRI fold chains in the outer circuit: plonky2's ArithmeticExtensionGate, ExponentiationGate and CosetInterpolationGate as gate programs,
and a circuit that proves what fri_verifier_query_round does for every query after the Merkle paths (fri/recursive_verifier.rs, recalled).

  arithmetic_ext_gate       2 constraints per op:  output - (c0 a b + c1 c)  over F[X]/(X^2 - W), limb by limb
  exponentiation_gate       n_bits + 1 constraints:  prev^2 (bit base + 1 - bit) - intermediate_i,  output - last intermediate
  coset_interpolation_gate  shifted shift - point; per chunk the computed (eval, product) minus their wires; the last eval minus the
                            evaluation value -- every constraint expanded into base-field monomials, the domain points x_i = g^i and the
                            barycentric weights w_i = g^i / n folded into the coefficients
  arithmetic_row            an ArithmeticExt row of a circuit under construction (this circuit's and sipp_amd/fri_initial.py's)
  index_and_x, x_from_bits, fold_rounds_into, final_poly_into
                            the wiring of one query on any builder, its sources given as arguments: this circuit's queries, the x
                            of sipp_amd/fri_initial.py and the queries of sipp_amd/fri_verifier.py
  FriFoldCircuit            the statement "every query's fold chain leads from its first value to the final polynomial" as calls of
                            sipp_amd/circuit.py's CircuitBuilder, which makes the rows, the copy cycles (sigmas), the generators and
                            the level schedule of it
  FriFoldProver             the circuit through the library's CircuitData: built once, then prove(fold data) / verify

Layouts are the generators' (include/sipp_hip.h, SIPP_GEN_ARITHMETIC_EXT / _EXPONENTIATION / _COSET_INTERPOLATION).

Statement layout.  Public inputs = beta_r (ext) per round || the final polynomial (ext coefficients) || per query (x_index, the value `old`
entering the first fold (ext), the 2^arity_bits ext evals of every round).  They are hashed in circuit by the swap-0 Poseidon chain and
tied to the PublicInput gate (CircuitBuilder.hash_public_inputs).  Per query: a BaseSum row (1-bit limbs) splits x_index; an Exponentiation
row raises omega_M to rev(x_index) (its bit wires are the limbs in reverse order); an arithmetic op multiplies by the coset generator 7: x.
Per round: two RandomAccess copies check evals[within] = old limb by limb (their bit wires are the low limbs of the current index bits); an
Exponentiation row gives (g^-1)^rev(within), an arithmetic op multiplies it by x: the shift; a CosetInterpolation row takes the evals in
bit-reversed order and beta_r, its evaluation value is the next `old`; arity_bits squarings of x; the index drops its low arity_bits bits.
ArithmeticExt rows then evaluate the final polynomial at (x, 0) by Horner; the result is the last `old`.

Out of scope: fri_combine_initial (the first `old` is a public input; sipp_amd/fri_initial.py proves it); the Merkle paths of the opened cosets (MerkleOpeningCircuit's job);
the proof of work; mixed arities (one arity for every round: plonky2's ConstantArityBits).

numpy only; imports nothing from the test oracle."""
import numpy as np

from .circuit import (BASE_SUM, GEN_ARITHMETIC_EXT, GEN_COSET_INTERPOLATION, GEN_EXPONENTIATION, GEN_RANDOM_ACCESS, P, PUBLIC_INPUT,
                      CircuitBuilder, CircuitProver, _K, _W, _root_of_unity, _words, pi, random_access_into)
from .merkle import declare_swap_gate

EXT_W = 7                                       # X^2 = 7
COSET_GEN = 7                                   # the LDE coset's shift
MAX_MONOMIALS, MAX_FACTORS = 4096, 64           # the constraint interpreter's limits
GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "ArithmeticExt", "RandomAccess", "Exponentiation", "PoseidonSwap", "CosetInterpolation"]
GATE_GROUP = (0, 0, 0, 0, 0, 1, 1, 2, 3)        # the selector group of every gate
ARITHMETIC_EXT, RANDOM_ACCESS, EXPONENTIATION, POSEIDON_SWAP, COSET_INTERPOLATION = range(4, 9)
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


def arithmetic_ext_into(pr, n_ops, c0, c1, W):
    for k in range(n_ops):
        b = 8 * k
        a0, a1, m0, m1 = (_W, b), (_W, b + 1), (_W, b + 2), (_W, b + 3)
        for monos in ([(1, [(_W, b + 6)]), (-1, [(_K, c0), a0, m0]), (-W, [(_K, c0), a1, m1]), (-1, [(_K, c1), (_W, b + 4)])],
                      [(1, [(_W, b + 7)]), (-1, [(_K, c0), a0, m1]), (-1, [(_K, c0), a1, m0]), (-1, [(_K, c1), (_W, b + 5)])]):
            pr.constraint(monos)


def exponentiation_into(pr, n_bits):
    base = (_W, 0)
    for i in range(n_bits):
        bit, inter = (_W, n_bits - i), (_W, 2 + n_bits + i)
        sq = [(_W, 1 + n_bits + i)] * 2 if i else []                     # prev^2; prev_0 = 1
        pr.constraint([(1, sq + [bit, base]), (1, sq), (-1, sq + [bit]), (-1, [inter])])
    pr.constraint([(1, [(_W, 1 + n_bits)]), (-1, [(_W, 1 + 2 * n_bits)])])


def coset_interpolation_into(pr, s, d, W):
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


def arithmetic_ext_gate(n_ops, c0, c1, W=EXT_W):
    """ArithmeticExtensionGate: per op at b = 8k the two limbs of  output - (const[c0] a b + const[c1] c);  degree 3"""
    assert n_ops >= 1 and W % P
    pr, words = _words(arithmetic_ext_into, n_ops, c0, c1, W)
    assert pr.count == 2 * n_ops
    return words


def exponentiation_gate(n_bits):
    """ExponentiationGate: prev^2 (bit base + 1 - bit) - intermediate_i for the bits from the top wire down (prev_0 = 1), then
    output - last intermediate; no booleanity (upstream's gate has none); degree 4"""
    assert 1 <= n_bits <= 64
    pr, words = _words(exponentiation_into, n_bits)
    assert pr.count == n_bits + 1
    return words


def coset_interpolation_gate(s, d, W=EXT_W):
    """CosetInterpolationGate over the subgroup of order 2^s with chunks of degree d: 2 + 4 ni + 2 constraints, degree min(d, 2^s)"""
    assert 1 <= s <= 4 and d >= 2 and W % P
    pr, words = _words(coset_interpolation_into, s, d, W)
    assert pr.count == 4 + 4 * interpolation_layout(s, d)["ni"]
    return words


def declare_arithmetic_ext(b, index, kind=GEN_ARITHMETIC_EXT):
    """one arithmetic op over builder b's two constant columns as gate `index`; kind: the generator that fills its rows"""
    b.declare(index, 3, (kind, 1, b.k0, b.k1, EXT_W), arithmetic_ext_into, 1, b.k0, b.k1, EXT_W)


def arithmetic_row(b, a, m, c, c0, c1):
    """an ArithmeticExt row  c0 a m + c1 c  of builder b: operands are pairs of limb sources, None leaves an operand's cells free (its
    constant is 0) -> (the row, the output's cells)"""
    r = b.new_row(ARITHMETIC_EXT, c0, c1)
    b.place(r, [(2 * i + l, op[l]) for i, op in enumerate((a, m, c)) if op for l in range(2)])
    return r, ((6, r), (7, r))


def index_and_x(b, exp_gate, index, omega, zero, operands):
    """One query's reading of its index on builder b: a BaseSum row splits the source `index` into b.log_m bits; an Exponentiation row
    raises omega_M (the cell `omega`) to rev(index); an arithmetic op multiplies by the coset generator 7.  operands: what the op's unused
    a and m are fed (None: free cells).  -> (the three rows, the bit cells low first, x as an extension pair of cells)"""
    bs = b.new_row(BASE_SUM)
    b.place(bs, [(0, index)])
    bits = [(1 + i, bs) for i in range(b.log_m)]
    e0, xr, x = x_from_bits(b, exp_gate, bits, omega, zero, operands)
    return bs, e0, xr, bits, x


def x_from_bits(b, exp_gate, bits, omega, zero, operands):
    """index_and_x behind the split: the b.log_m bit cells (low first) are the caller's, whatever row split them
    -> (the Exponentiation row, the arithmetic row, x as an extension pair of cells)"""
    M = b.log_m
    # omega_M ^ rev(x_index): exponent bit j = index bit M - 1 - j
    e0 = b.new_row(exp_gate)
    b.place(e0, [(0, omega)] + [(1 + j, bits[M - 1 - j]) for j in range(M)])
    # x = 7 (omega_M ^ rev, 0): the c operand
    xr, x = arithmetic_row(b, operands, operands, ((1 + M, e0), zero), 0, COSET_GEN)
    return e0, xr, x


def fold_rounds_into(b, gates, ra_stride, zero, ginv, bits, x, old, ev, beta, within=None):
    """The fold chain of one query on builder b (b.n_rounds rounds of arity 2^b.arity_bits).  gates = (RandomAccess with two copies of
    2^arity_bits items at ra_stride, Exponentiation, CosetInterpolation); bits: the index bit cells, low first; x: the cell of the
    query's point; old: the two limb sources of the value entering round 0; ev(r, j, l): the source of limb l of evaluation j of round
    r, natural order; beta(r, l): the source of limb l of round r's challenge; within(r): the source of round r's RandomAccess index
    (None: the two index cells stay free input cells).
    -> ((the RandomAccess, exponentiation, shift, interpolation rows, the squaring rows per round), the last x, the last old)"""
    ra_gate, exp_gate, interp_gate = gates
    a, A, M, it = b.arity_bits, b.arity, b.log_m, b.interp
    ras, exs, sfs, its, sqs = [], [], [], [], []
    for r in range(b.n_rounds):
        # evals[within] = old, limb by limb; the index is an input, the bit wires are the low limbs of the current index bits
        # (generators write the claimed element and the bits on both sides: no copies)
        ra = b.new_row(ra_gate)
        feeds = []
        for l in range(2):
            at = ra_stride * l
            b.tie(old[l], (at + 1, ra))
            feeds += ([(at, within(r))] if within else []) + [(at + 2 + j, ev(r, j, l)) for j in range(A)]
            for t in range(a):
                b.tie(bits[t], (at + 2 + A + t, ra))
        b.place(ra, feeds)
        # (g^-1) ^ rev(within): exponent bit j = index bit a - 1 - j, the bits above are 0
        ex = b.new_row(exp_gate)
        b.place(ex, [(0, ginv)] + [(1 + j, bits[a - 1 - j] if j < a else zero) for j in range(M)])
        # shift = (g^-1)^rev x
        sf, shift = arithmetic_row(b, ((1 + M, ex), zero), (x, zero), None, 1, 0)
        # the interpolation at beta_r of the evals in bit-reversed order
        ir = b.new_row(interp_gate)
        feeds = [(it["shift"], shift[0])] + [(it["point"] + l, beta(r, l)) for l in range(2)]
        feeds += [(it["values"] + 2 * k + l, ev(r, reverse_bits(k, a), l)) for k in range(A) for l in range(2)]
        b.place(ir, feeds)
        old = [(it["eval"], ir), (it["eval"] + 1, ir)]
        # x <- x^arity
        sq = []
        for _ in range(a):
            row, (x, _) = arithmetic_row(b, (x, zero), (x, zero), None, 1, 0)
            sq.append(row)
        bits = bits[a:]
        ras.append(ra); exs.append(ex); sfs.append(sf); its.append(ir); sqs.append(sq)
    return (ras, exs, sfs, its, sqs), x, old


def final_poly_into(b, zero, x, coeff):
    """the final polynomial (b.final_len coefficients, coeff(k, l) = the source of limb l of coefficient k) at (x, 0) by Horner:
    acc = c_(F-1); acc <- acc (x, 0) + c_k  -> (the rows, the result's two limb sources)"""
    F = b.final_len
    acc, rows = [coeff(F - 1, l) for l in range(2)], []
    for k in range(F - 2, -1, -1):
        row, acc = arithmetic_row(b, acc, (x, zero), [coeff(k, l) for l in range(2)], 1, 1)
        rows.append(row)
    return rows, acc


class FriFoldCircuit(CircuitBuilder):
    """The circuit of the fold chains of n_queries queries of a FRI opening proof over an LDE of 2^log_m points: n_rounds rounds of arity
    2^arity_bits, a final polynomial of final_len ext coefficients.  Cells are wire * N + row."""
    n_public_args = 3

    def __init__(self, log_m, arity_bits, n_rounds, final_len, n_queries, num_wires=135, num_routed=80, min_log_n=10):
        assert 1 <= arity_bits <= 4 and n_rounds >= 1 and arity_bits * n_rounds <= log_m <= 64 and final_len >= 1 and n_queries >= 1
        assert 2 + 2 * log_m <= num_wires and 2 + log_m <= num_routed and num_wires >= 135
        self.log_m, self.arity_bits, self.n_rounds, self.final_len, self.n_queries = log_m, arity_bits, n_rounds, final_len, n_queries
        self.arity = 1 << arity_bits
        super().__init__(num_wires, num_routed, GATE_NAMES, GATE_GROUP, 2,
                         2 * n_rounds + 2 * final_len + n_queries * (3 + 2 * self.arity * n_rounds))
        self.ra_stride = 2 + self.arity + arity_bits
        assert self.ra_stride + 2 + self.arity + arity_bits <= num_routed
        self.interp = interpolation_layout(arity_bits, INTERP_DEGREE)
        assert self.interp["point"] + 4 <= num_routed and self.interp["num_wires"] <= num_wires
        self.omega_m = _root_of_unity(log_m)
        self.g_inv = pow(_root_of_unity(arity_bits), P - 2, P)
        self.declare_basic(log_m)
        declare_arithmetic_ext(self, ARITHMETIC_EXT)
        self.declare(RANDOM_ACCESS, arity_bits + 1, (GEN_RANDOM_ACCESS, 2, self.ra_stride, arity_bits), random_access_into, 2, self.ra_stride,
                     arity_bits)
        self.declare(EXPONENTIATION, 4, (GEN_EXPONENTIATION, log_m), exponentiation_into, log_m)
        declare_swap_gate(self, POSEIDON_SWAP)
        self.declare(COSET_INTERPOLATION, min(INTERP_DEGREE, self.arity), (GEN_COSET_INTERPOLATION, arity_bits, INTERP_DEGREE, EXT_W),
                     coset_interpolation_into, arity_bits, INTERP_DEGREE, EXT_W)
        self._wiring()
        self.finish(min_log_n)
        # the input cells the partial witness sets besides the public inputs' cycles: per query and round the RandomAccess indices (`within`)
        self.input_cells = [[[self.ra_stride * l * self.n + ra for l in range(2)] for ra in rows] for rows in self.ra_row]

    # public-input positions
    def pi_beta(self, r, l):
        return 2 * r + l

    def pi_final(self, k, l):
        return 2 * self.n_rounds + 2 * k + l

    def pi_query(self, q):
        return 2 * self.n_rounds + 2 * self.final_len + q * (3 + 2 * self.arity * self.n_rounds)

    def pi_eval(self, q, r, j, l):
        return self.pi_query(q) + 3 + 2 * (self.arity * r + j) + l

    def _wiring(self):
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.omega_row, omega = self.constant(self.omega_m)
        self.ginv_row, ginv = self.constant(self.g_inv)
        self.bs_row, self.exp0_row, self.x_row, self.ra_row, self.exp_row, self.shift_row, self.interp_row, self.sq_row, self.horner_row = (
            [], [], [], [], [], [], [], [], [])
        gates = (RANDOM_ACCESS, EXPONENTIATION, COSET_INTERPOLATION)
        for q in range(self.n_queries):
            base = self.pi_query(q)
            bs, e0, xr, bits, (x, _) = index_and_x(self, EXPONENTIATION, pi(base), omega, zero, None)
            self.bs_row.append(bs); self.exp0_row.append(e0); self.x_row.append(xr)
            # the first old = the claimed element of round 0
            rows, x, old = fold_rounds_into(self, gates, self.ra_stride, zero, ginv, bits, x, [pi(base + 1), pi(base + 2)],
                                            lambda r, j, l: pi(self.pi_eval(q, r, j, l)), lambda r, l: pi(self.pi_beta(r, l)))
            for have, got in zip((self.ra_row, self.exp_row, self.shift_row, self.interp_row, self.sq_row), rows):
                have.append(got)
            rows, acc = final_poly_into(self, zero, x, lambda k, l: pi(self.pi_final(k, l)))
            self.horner_row.append(rows)
            for l in range(2):
                self.tie(acc[l], old[l])
        self.hash_public_inputs(POSEIDON_SWAP, zero)

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
        w, flat = self.public_input_witness(self.public_inputs(betas, final_poly, queries))
        for q, (x_index, _, _) in enumerate(self._check(betas, final_poly, queries)[2]):
            for r in range(self.n_rounds):
                within = (x_index >> (self.arity_bits * r)) & (self.arity - 1)
                flat[np.asarray(self.input_cells[q][r], dtype=np.int64)] = np.uint64(within)
        return w


class FriFoldProver(CircuitProver):
    """FriFoldCircuit through the library's CircuitData: built once, then prove(betas, final_poly, queries) / verify"""

    def __init__(self, ctx, log_m, arity_bits, n_rounds, final_len, n_queries, fri=None, params=None, digest=None, min_log_n=10):
        super().__init__(ctx, FriFoldCircuit(log_m, arity_bits, n_rounds, final_len, n_queries, min_log_n=min_log_n), fri, params, digest)
