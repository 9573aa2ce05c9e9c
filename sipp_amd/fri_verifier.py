"""One FRI query round in the outer circuit: the Merkle openings (sipp_amd/merkle.py), the initial combination (sipp_amd/fri_initial.py) and
the fold chain (sipp_amd/fri_fold.py) wired on ONE builder, each handing the next its cells: plonky2's verify_fri_proof after its
challenges are drawn (fri/recursive_verifier.rs, recalled), for an opening proof of sipp_fri_prove_openings.

  FriQueryRoundCircuit   the statement "every query round of this opening proof verifies against these caps" as calls of the three
                         modules' wiring routines (opening_into; openings_into, combine_into; x_from_bits, fold_rounds_into,
                         final_poly_into) on sipp_amd/circuit.py's CircuitBuilder
  query_rounds_into      that wiring with what the challenges decide given as sources (alpha, beta_r, the index bits, the cap index,
                         within(r)): this class's public and witness inputs, or the cells sipp_amd/fri_proof.py draws in circuit
  proof_arguments        the proof's data as a caller has it -> the argument tuple of public_inputs / partial_witness / input_cells / prove
  FriVerifierProver      the circuit through the library's CircuitData: built once, then prove(arguments) / verify; the proof is made
                         from the input cells alone (sipp_circuit_prove_inputs), not from a dense table

Statement, per query.  Initial openings: for every initial oracle the opened row sits at leaf x_index under that oracle's cap (leaf
hash by hash_or_noop, log_m - cap_height swap rows, RandomAccess selects cap[x_index >> height]).  Initial combination: the columns of
those same row cells, in the order of `batches`, combine with the claimed openings into fri_combine_initial; times x this is the first
`old`.  Folds: round r's 2^arity_bits evaluations are the leaf at index x_index >> (arity_bits (r + 1)) of the tree under round r's
cap (the leaf holds the evaluations' limbs in the proof's order); evals[within] = old; the interpolation at beta_r gives the next old.
Final polynomial: at x it equals the last old.

Public inputs = alpha (ext) || per batch (the point (ext), its opened values (ext each)) || per initial oracle its cap (2^cap_height
digests, flat) || per round (its cap, beta_r (ext)) || the final polynomial (ext coefficients) || x_index per query.  They are hashed in
circuit by the swap-0 Poseidon chain and tied to the PublicInput gate (CircuitBuilder.hash_public_inputs).  Everything else the proof
carries is a witness input (CircuitBuilder.witness_input) that only the constraints bind: the opened rows, every sibling, every
round's evaluations, the RandomAccess indices.

One reading of the index and of x per query: one BaseSum split of x_index into log_m bits feeds the swap wires of every path (round r's
tree from bit arity_bits (r + 1) up), the `within` bits of every round, the exponent of omega_M and the bit wires of every cap
selection (the top cap_height bits: one cap index per query serves every tree); one Exponentiation row and one arithmetic op give x
for the combination's denominators and the fold chain.  One cell per evaluation is the source of its three uses: the leaf hash in the
proof's order, the interpolation row in bit-reversed order, the RandomAccess items in natural order.

Edges.  A leaf of at most 4 values is its own digest, padded with zero: no hash rows (narrow oracles; coset leaves at arity_bits = 1).
A commit-phase tree with exactly 2^cap_height leaves has no swap row: its leaf digest is the cap selection's claimed words.

Refused at build: mixed arities (arity_bits given per round with different values); salted (hiding) oracles (n_salt); empty batches;
and in THIS class the proof of work (pow_bits != 0) and drawing the challenges in circuit (draw_challenges), which
sipp_amd/fri_proof.py's FriProofCircuit does around the same wiring (query_rounds_into).  Merkle paths are climbed with the Poseidon gate:
trees hashed with Keccak (SIPP_HASH_KECCAK25) are not verified here, and a witness from such a proof satisfies no row.

numpy only; imports nothing from the test oracle."""
import numpy as np

from .circuit import (BASE_SUM, GEN_EXPONENTIATION, GEN_QUOTIENT_EXT, GEN_RANDOM_ACCESS, GEN_REDUCING, GEN_REDUCING_EXT, GEN_COSET_INTERPOLATION, P,
                      PUBLIC_INPUT, CircuitBuilder, CircuitProver, _root_of_unity, pi, random_access_into)
from .fri_fold import (ARITHMETIC_EXT, EXT_W, INTERP_DEGREE, coset_interpolation_into, declare_arithmetic_ext, exponentiation_into,
                       final_poly_into, fold_rounds_into, interpolation_layout, x_from_bits)
from .fri_initial import _reducing_into, combine_into, openings_into
from .merkle import declare_swap_gate, opening_into

GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "ArithmeticExt", "Reducing", "ReducingExt", "QuotientExt", "Exponentiation",
              "RandomAccessCap", "RandomAccessEval", "PoseidonSwap", "CosetInterpolation"]
REDUCING, REDUCING_EXT, QUOTIENT_EXT, EXPONENTIATION, RANDOM_ACCESS_CAP, RANDOM_ACCESS_EVAL, POSEIDON_SWAP, COSET_INTERPOLATION = range(5, 13)


def gate_groups(cap_height, arity_bits):
    """the selector group of every gate: filter degree (gates in the group) plus gate degree stays within 8.  Group 0: the five gates
    of degree <= 3; group 1: the four of degree <= 4; the two RandomAccess shapes (degrees cap_height + 1, arity_bits + 1) share a group
    where 2 + the larger degree allows it; PoseidonSwap (7) and CosetInterpolation (up to 7) stand alone"""
    if 2 + max(cap_height, arity_bits) + 1 <= 8:
        return (0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 4)
    return (0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 4, 5)


ROW_NAMES = ("bs_row", "exp0_row", "x_row", "init_ra_row", "init_hash_row", "init_path_row", "reduce_row", "num_row", "den_row", "quot_row",
             "total_row", "old_row", "ra_row", "exp_row", "shift_row", "interp_row", "sq_row", "coset_ra_row", "coset_hash_row",
             "coset_path_row", "horner_row")


def query_rounds_into(c, consts, alpha, beta, bits_of, cap_index_of, within_of, opened=None, cap=None, round_cap=None, point=None, final=None):
    """Every query round of circuit c (a FriQueryRoundCircuit, or sipp_amd/fri_proof.py's circuit of the same shape attributes and public-
    input positions) with what the challenges decide given as arguments.  consts = the cells (zero, one, omega_M, 1 / g); alpha: two limb
    sources; beta(r, l): the source of limb l of round r's challenge; bits_of(q) -> (the row that split query q's index, its log_m bit
    cells, low first); cap_index_of(q, bits) -> the source of the index's top cap_height bits as one value; within_of(q, r, bits) -> the
    source of round r's index within its coset (bits: the arity_bits cells it is made of).  The opened rows, the siblings, the
    evaluations and the coset siblings are witness inputs made here (c._new_input).  Sets c.opened_row, c.power_row and the per-query
    row lists ROW_NAMES.
    What the proof and its statement carry besides are sources too: opened(b, j, l) = limb l of batch b's opened value j; cap(o, j, w) =
    word w of digest j of initial oracle o's cap; round_cap(r, j, w) the same of round r's cap; point(b, l) = limb l of batch b's point;
    final(k, l) = limb l of the final polynomial's coefficient k.  None = c's public input at c.pi_opened / pi_cap / pi_round_cap /
    pi_point / pi_final: a circuit that holds them elsewhere (witness inputs, cells drawn in circuit) passes its own."""
    zero, one, omega, ginv = consts
    opened = opened or (lambda b, j, l: pi(c.pi_opened(b, j, l)))
    cap = cap or (lambda o, j, w: pi(c.pi_cap(o, j, w)))
    round_cap = round_cap or (lambda r, j, w: pi(c.pi_round_cap(r, j, w)))
    point = point or (lambda b, l: pi(c.pi_point(b, l)))
    final = final or (lambda k, l: pi(c.pi_final(k, l)))
    a, M, C = c.arity_bits, c.log_m, c.cap_height
    cap_shape = (RANDOM_ACCESS_CAP, c.cap_rows, c.cap_copies, c.cap_stride, c.n_cap)
    # once per proof and batch: the reduced openings, alpha^len
    c.opened_row, c.power_row, acc_o, alpha_len = openings_into(c, REDUCING_EXT, alpha, zero, opened)
    for name in ROW_NAMES:
        setattr(c, name, [])
    for q in range(c.n_queries):
        # the one reading of the index and of x
        bs, bits = bits_of(q)
        e0, xr, x = x_from_bits(c, EXPONENTIATION, bits, omega, zero, None)
        cap_index, cap_bits = cap_index_of(q, bits[M - C:]), bits[M - C:]
        # the initial openings: every oracle's row under its cap
        leaves, ras, hashes, paths = [], [], [], []
        for o, width in enumerate(c.oracle_widths):
            row = [c._new_input("row", q, o, k) for k in range(width)]
            sib = [[c._new_input("sibling", q, o, l, t) for t in range(4)] for l in range(c.height)]
            ra, hs, path = opening_into(c, cap_shape, POSEIDON_SWAP, zero, row, bits[:c.height], cap_index,
                                        lambda j, w: cap(o, j, w), cap_bits, lambda l, t: sib[l][t])
            leaves += row
            ras.append(ra); hashes.append(hs); paths.append(path)
        # the combination of those same row cells, times x: the first old
        (lf, nm, dn, qt, tt, orow), old = combine_into(c, (REDUCING, QUOTIENT_EXT), alpha, zero, one, x, acc_o, alpha_len,
                                                       lambda k: leaves[k], point)
        # the folds: one cell per evaluation for the RandomAccess items, the interpolation row and (below) the coset leaf
        ev = [[[c._new_input("eval", q, r, j, l) for l in range(2)] for j in range(c.arity)] for r in range(c.n_rounds)]
        within = [within_of(q, r, bits[a * r:a * (r + 1)]) for r in range(c.n_rounds)]
        fold_rows, x_last, last = fold_rounds_into(c, (RANDOM_ACCESS_EVAL, EXPONENTIATION, COSET_INTERPOLATION), c.ra_stride, zero,
                                                   ginv, bits, x[0], list(old), lambda r, j, l: ev[r][j][l], beta, lambda r: within[r])
        # every round's evaluations are a leaf under that round's cap, in the proof's order
        cras, chashes, cpaths = [], [], []
        for r in range(c.n_rounds):
            sib = [[c._new_input("coset_sibling", q, r, l, t) for t in range(4)] for l in range(c.round_height[r])]
            ra, hs, path = opening_into(c, cap_shape, POSEIDON_SWAP, zero, [ev[r][j][l] for j in range(c.arity) for l in range(2)],
                                        bits[a * (r + 1):M - C], cap_index, lambda j, w: round_cap(r, j, w), cap_bits,
                                        lambda l, t: sib[l][t])
            cras.append(ra); chashes.append(hs); cpaths.append(path)
        # the final polynomial at x is the last old
        horner, acc = final_poly_into(c, zero, x_last, final)
        for l in range(2):
            c.tie(acc[l], last[l])
        for name, got in zip(ROW_NAMES, (bs, e0, xr, ras, hashes, paths, lf, nm, dn, qt, tt, orow) + tuple(fold_rows) + (cras, chashes, cpaths, horner)):
            getattr(c, name).append(got)


class FriQueryRoundCircuit(CircuitBuilder):
    """The circuit of the n_queries query rounds of a FRI opening proof over an LDE of 2^log_m points: initial oracles of
    oracle_widths[o] columns under caps of 2^cap_height digests; batch b combines the columns batches[b] (indices into the row of all
    oracles' columns, concatenated, in the order of the batch's opened values); n_rounds rounds of arity 2^arity_bits; a final
    polynomial of final_len ext coefficients.  Cells are wire * N + row."""
    n_public_args = 8                                           # public_inputs takes partial_witness's arguments without the queries

    def __init__(self, log_m, cap_height, oracle_widths, batches, arity_bits, n_rounds, final_len, n_queries, num_wires=135, num_routed=80,
                 k_base=None, k_ext=None, min_log_n=10, pow_bits=0, draw_challenges=False, n_salt=None):
        assert pow_bits == 0, "the proof of work is out of scope"
        assert not draw_challenges, "drawing the challenges in circuit (the challenger) is out of scope"
        self._set_shape(log_m, cap_height, oracle_widths, batches, arity_bits, n_rounds, final_len, n_queries, num_wires, num_routed, k_base,
                        k_ext, n_salt)
        # public-input positions
        self.pi_batch, t = [], 2
        for b in self.batches:
            self.pi_batch.append(t)
            t += 2 + 2 * len(b)
        self.pi_caps = t
        self.pi_rounds = t + 4 * self.n_cap * len(self.oracle_widths)
        self.pi_finals = self.pi_rounds + n_rounds * (4 * self.n_cap + 2)
        self.pi_queries = self.pi_finals + 2 * final_len
        CircuitBuilder.__init__(self, num_wires, num_routed, GATE_NAMES, gate_groups(cap_height, self.arity_bits), 2, self.pi_queries + n_queries)
        self._declare_gates()
        self._in_keys = []                                      # what every witness input is, in the order of their making
        self._wiring()
        self.finish(min_log_n)
        cells = [x for cyc in self.pi_cycle + self.in_cycle for x in cyc]
        assert len(cells) == len(set(cells))

    def _set_shape(self, log_m, cap_height, oracle_widths, batches, arity_bits, n_rounds, final_len, n_queries, num_wires, num_routed, k_base,
                   k_ext, n_salt):
        """the shape's refusals and what the wiring reads of it (sipp_amd/fri_proof.py's circuit takes the same shapes)"""
        if not isinstance(arity_bits, int):
            arity_bits = [int(a) for a in arity_bits]
            assert len(arity_bits) == n_rounds and len(set(arity_bits)) == 1, "mixed arities are out of scope"
            arity_bits = arity_bits[0]
        oracle_widths = [int(w) for w in oracle_widths]
        assert not any(n_salt or ()), "salted (hiding) oracles are out of scope"
        batches = [[int(c) for c in b] for b in batches]
        assert batches and all(len(b) >= 1 for b in batches), "an empty batch is out of scope"
        n_columns = sum(oracle_widths)
        assert oracle_widths and all(w >= 1 for w in oracle_widths) and all(0 <= c < n_columns for b in batches for c in b)
        assert 1 <= arity_bits <= 4 and n_rounds >= 1 and final_len >= 1 and n_queries >= 1 and 1 <= cap_height <= 6
        # every commit-phase tree has at least its cap's leaves
        assert arity_bits * n_rounds + cap_height <= log_m <= 64
        assert 2 + 2 * log_m <= num_wires and 2 + log_m <= num_routed and num_wires >= 135
        k_base = (num_routed - 4) // 3 if k_base is None else k_base
        k_ext = (num_routed - 4) // 4 if k_ext is None else k_ext
        assert k_base >= 1 and 3 * k_base + 4 <= num_routed and k_ext >= 1 and 4 * k_ext + 4 <= num_routed
        self.log_m, self.cap_height, self.oracle_widths, self.batches, self.n_columns = log_m, cap_height, oracle_widths, batches, n_columns
        self.arity_bits, self.n_rounds, self.final_len, self.n_queries, self.k_base, self.k_ext = arity_bits, n_rounds, final_len, n_queries, k_base, k_ext
        self.arity, self.n_cap = 1 << arity_bits, 1 << cap_height
        self.height = log_m - cap_height                                               # of an initial tree
        self.round_height = [self.height - arity_bits * (r + 1) for r in range(n_rounds)]
        self.omega_m = _root_of_unity(log_m)
        self.g_inv = pow(_root_of_unity(arity_bits), P - 2, P)
        # cap selection: per copy index, claimed, 2^cap_height items, cap_height bits, all routed (the bits are tied to the index split);
        # copies per row divide 4 (one digest word per copy)
        self.cap_stride = 2 + self.n_cap + cap_height
        self.cap_copies = next(c for c in (4, 2, 1) if c * self.cap_stride <= num_routed)
        self.cap_rows = 4 // self.cap_copies
        # evaluation selection: two copies (the limbs) of 2^arity_bits items
        self.ra_stride = 2 + self.arity + arity_bits
        assert 2 * self.ra_stride <= num_routed
        self.interp = interpolation_layout(arity_bits, INTERP_DEGREE)
        assert self.interp["point"] + 4 <= num_routed and self.interp["num_wires"] <= num_wires

    def _declare_gates(self):
        """the thirteen gates of GATE_NAMES"""
        log_m, cap_height, arity_bits, k_base, k_ext = self.log_m, self.cap_height, self.arity_bits, self.k_base, self.k_ext
        self.declare_basic(log_m)
        declare_arithmetic_ext(self, ARITHMETIC_EXT)
        self.declare(REDUCING, 2, (GEN_REDUCING, k_base, EXT_W), _reducing_into, k_base, EXT_W, False)
        self.declare(REDUCING_EXT, 2, (GEN_REDUCING_EXT, k_ext, EXT_W), _reducing_into, k_ext, EXT_W, True)
        declare_arithmetic_ext(self, QUOTIENT_EXT, GEN_QUOTIENT_EXT)
        self.declare(EXPONENTIATION, 4, (GEN_EXPONENTIATION, log_m), exponentiation_into, log_m)
        self.declare(RANDOM_ACCESS_CAP, cap_height + 1, (GEN_RANDOM_ACCESS, self.cap_copies, self.cap_stride, cap_height), random_access_into,
                     self.cap_copies, self.cap_stride, cap_height)
        self.declare(RANDOM_ACCESS_EVAL, arity_bits + 1, (GEN_RANDOM_ACCESS, 2, self.ra_stride, arity_bits), random_access_into, 2, self.ra_stride,
                     arity_bits)
        declare_swap_gate(self, POSEIDON_SWAP)
        self.declare(COSET_INTERPOLATION, min(INTERP_DEGREE, self.arity), (GEN_COSET_INTERPOLATION, arity_bits, INTERP_DEGREE, EXT_W),
                     coset_interpolation_into, arity_bits, INTERP_DEGREE, EXT_W)

    # public-input positions
    def pi_alpha(self, l):
        return l

    def pi_point(self, b, l):
        return self.pi_batch[b] + l

    def pi_opened(self, b, j, l):
        return self.pi_batch[b] + 2 + 2 * j + l

    def pi_cap(self, o, j, w):
        """word w of digest j of initial oracle o's cap"""
        return self.pi_caps + 4 * (self.n_cap * o + j) + w

    def pi_round_cap(self, r, j, w):
        return self.pi_rounds + r * (4 * self.n_cap + 2) + 4 * j + w

    def pi_beta(self, r, l):
        return self.pi_rounds + r * (4 * self.n_cap + 2) + 4 * self.n_cap + l

    def pi_final(self, k, l):
        return self.pi_finals + 2 * k + l

    def pi_x_index(self, q):
        return self.pi_queries + q

    def _new_input(self, *key):
        self._in_keys.append(key)
        return self.witness_input()

    def _wiring(self):
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.one_row, one = self.constant(1)
        self.omega_row, omega = self.constant(self.omega_m)
        self.ginv_row, ginv = self.constant(self.g_inv)
        alpha = (pi(self.pi_alpha(0)), pi(self.pi_alpha(1)))

        def bits_of(q):                                         # the one reading of the index: a BaseSum row splits the public x_index
            bs = self.new_row(BASE_SUM)
            self.place(bs, [(0, pi(self.pi_x_index(q)))])
            return bs, [(1 + i, bs) for i in range(self.log_m)]
        query_rounds_into(self, (zero, one, omega, ginv), alpha, lambda r, l: pi(self.pi_beta(r, l)), bits_of,
                          lambda q, bits: self._new_input("cap_index", q), lambda q, r, bits: self._new_input("within", q, r))
        self.hash_public_inputs(POSEIDON_SWAP, zero)

    # ---- the values ----
    def _check(self, alpha, points, opened, caps, round_caps, betas, final_poly, x_indices, queries=None):
        ext = lambda v: (int(v[0]) % P, int(v[1]) % P)
        nb, no, R, A = len(self.batches), len(self.oracle_widths), self.n_rounds, self.arity
        assert len(points) == nb == len(opened) and all(len(v) == len(b) for v, b in zip(opened, self.batches))
        caps = [np.asarray(c, dtype=np.uint64).reshape(self.n_cap, 4) for c in caps]
        round_caps = [np.asarray(c, dtype=np.uint64).reshape(self.n_cap, 4) for c in round_caps]
        assert len(caps) == no and len(round_caps) == R == len(betas) and len(final_poly) == self.final_len
        x_indices = [int(x) for x in x_indices]
        assert len(x_indices) == self.n_queries and all(0 <= x < (1 << self.log_m) for x in x_indices)
        out = (ext(alpha), [ext(p) for p in points], [[ext(v) for v in vals] for vals in opened], caps, round_caps, [ext(b) for b in betas],
               [ext(c) for c in final_poly], x_indices)
        if queries is None:
            return out
        assert len(queries) == self.n_queries
        checked = []
        for rows, siblings, evals, coset_siblings in queries:
            rows = [[int(v) % P for v in row] for row in rows]
            assert [len(row) for row in rows] == self.oracle_widths
            siblings = [np.asarray(s, dtype=np.uint64).reshape(self.height, 4) for s in siblings]
            evals = [[ext(v) for v in rnd] for rnd in evals]
            assert len(siblings) == no and len(evals) == R == len(coset_siblings) and all(len(rnd) == A for rnd in evals)
            coset_siblings = [np.asarray(s, dtype=np.uint64).reshape(self.round_height[r], 4) for r, s in enumerate(coset_siblings)]
            checked.append((rows, siblings, evals, coset_siblings))
        return out + (checked,)

    def public_inputs(self, alpha, points, opened, caps, round_caps, betas, final_poly, x_indices):
        """alpha || per batch (point, opened values) || the initial caps || per round (cap, beta) || the final polynomial || the x_index of
        every query, as ints; ext values as (c0, c1) pairs"""
        alpha, points, opened, caps, round_caps, betas, final_poly, x_indices = self._check(alpha, points, opened, caps, round_caps, betas,
                                                                                            final_poly, x_indices)
        out = list(alpha)
        for pt, vals in zip(points, opened):
            out += list(pt) + [l for v in vals for l in v]
        for cap in caps:
            out += [int(v) for v in cap.reshape(-1)]
        for cap, beta in zip(round_caps, betas):
            out += [int(v) for v in cap.reshape(-1)] + list(beta)
        out += [l for c in final_poly for l in c] + x_indices
        assert len(out) == self.n_pi
        return out

    def witness_inputs(self, *args):
        """the value of every witness input, in the order of their making"""
        x_indices, queries = self._check(*args)[7:9]
        a, out = self.arity_bits, []
        for key in self._in_keys:
            kind, q = key[0], key[1]
            rows, siblings, evals, coset_siblings = queries[q]
            if kind == "cap_index":
                out.append(x_indices[q] >> self.height)
            elif kind == "row":
                out.append(rows[key[2]][key[3]])
            elif kind == "sibling":
                out.append(int(siblings[key[2]][key[3], key[4]]))
            elif kind == "eval":
                out.append(evals[key[2]][key[3]][key[4]])
            elif kind == "within":
                out.append((x_indices[q] >> (a * key[2])) & (self.arity - 1))
            else:
                out.append(int(coset_siblings[key[2]][key[3], key[4]]))
        return out

    def input_cells(self, *args):
        """(cells, values), uint64: every cell the partial witness sets, each once -- the cycles of the public inputs, then those of
        the witness inputs (cell = wire * N + row)"""
        vals = [v % P for v in self.public_inputs(*args[:self.n_public_args])] + self.witness_inputs(*args)
        cycles = self.pi_cycle + self.in_cycle
        cells = np.array([x for cyc in cycles for x in cyc], dtype=np.uint64)
        values = np.array([v for cyc, v in zip(cycles, vals) for _ in cyc], dtype=np.uint64)
        return cells, values

    def partial_witness(self, *args):
        """[num_wires][N] with the INPUT cells set (plonky2's PartialWitness as a dense table): input_cells scattered into zeros"""
        cells, values = self.input_cells(*args)
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        w.reshape(-1)[cells.astype(np.int64)] = values
        return w


def proof_arguments(caps, points, opened, alpha, round_caps, betas, final_poly, queries):
    """The data of one opening proof as a caller has it -> the argument tuple of FriQueryRoundCircuit.public_inputs (its first eight) /
    partial_witness / input_cells and of FriVerifierProver.prove.  caps: per initial oracle 2^cap_height digests; points, opened: per
    batch; alpha, betas, final_poly: ext values as (c0, c1); round_caps: per round; queries: per query (x_index, the opened row of every
    oracle, every oracle's siblings (4 words each, leaf upwards), per round the 2^arity_bits ext evaluations, per round the coset leaf's
    siblings)"""
    return (alpha, points, opened, caps, round_caps, betas, final_poly, [q[0] for q in queries], [tuple(q[1:5]) for q in queries])


class FriVerifierProver(CircuitProver):
    """FriQueryRoundCircuit through the library's CircuitData: built once, then prove(*proof_arguments(...)) / verify.  prove() hands the
    library the input cells as (cell, value) pairs (sipp_circuit_prove_inputs): no dense table is made or uploaded."""

    def __init__(self, ctx, *shape, fri=None, params=None, digest=None, **kw):
        super().__init__(ctx, FriQueryRoundCircuit(*shape, **kw), fri, params, digest)

    def prove(self, *inputs):
        c = self.circ
        cells, values = c.input_cells(*inputs)
        return self.data.prove_inputs(cells, values, c.public_inputs(*inputs[:c.n_public_args]))
