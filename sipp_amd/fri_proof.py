"""The whole of plonky2's verify_fri_proof in the outer circuit, for an opening proof of sipp_fri_prove_openings: the query rounds of
sipp_amd/fri_verifier.py (query_rounds_into) behind a challenger that runs IN CIRCUIT (plonky2's RecursiveChallenger, iop/challenger.rs,
recalled), with the proof of work.  alpha, every beta_r and every x_index are generated cells: nobody who asks for the proof picks them.

  FriProofCircuit   the statement "this opening proof verifies against these caps, behind this transcript"
  _proof_into       (a method of the circuit) the transcript, the proof of work and the queries behind a challenger that is handed in,
                    over sources: this circuit passes its public inputs, sipp_amd/plonk_verifier.py's joined circuit its own
  FriProofProver    the circuit through the library's CircuitData: the map from the proof's words to the input cells is fixed at build
                    (words_map) and set on the device once; prove_proof(flat proof, caps, points, transcript) sends the words and
                    calls sipp_circuit_prove_words (without a device map: a numpy gather and sipp_circuit_prove_inputs);
                    prove(*arguments) with explicit arguments stays, for tests and tampering

Challenger.  observe() buffers sources; eight buffered inputs, or a get() with inputs pending or no output left, make one swap-0
PoseidonSwap row whose first inputs are the buffered sources and whose other inputs are the outputs of the row before (the arriving
state for the first row); challenges pop from the end of the rate part; an observation discards pending outputs.  The existing
generator (SIPP_GEN_POSEIDON_SWAP) fills the rows.

Transcript, in sipp_fri_prove_openings' order: the opened values batch by batch; alpha; per round its cap, then beta_r; the final
polynomial; the proof of work; one challenge per query.  The ARRIVING transcript is 12 state words and n_in (0 .. 7, a build parameter)
pending input words, public inputs both; pending output needs nothing, the first observation discards it.

Proof of work, pow_bits 0 .. 32.  Rule 0: the witness is observed, the next challenge is the response.  Rule 1: the response is word 0
of hash_no_pad(get_hash() || witness), one more hash row.  The response is split into 64 one-bit limbs (gate BaseSplit64, generator
SIPP_GEN_BASE_SPLIT); its top pow_bits limbs are tied to the zero constant.

Query indices.  Each query's challenge goes through the same 64-limb split; the low log_m limbs are THE bit cells of the query (swap
wires, exponent, cap selections, every round's `within` bits).  The cap index is the le_sum of the top cap_height bits, round r's
RandomAccess index the le_sum of its arity_bits bits: BaseSum rows whose generator is SIPP_GEN_BASE_SUM (kind 15, limbs -> sum).
The 64-bit split of a field element is not unique: a value v < 2^32 - 1 is also the limbs of v + p.  plonky2's recursive verifier
accepts that (split_le of a challenge, fri/recursive_verifier.rs), and so does this circuit: a prover may take either reading of such
a challenge (or response), one chance in 2^32 per draw.  The generator writes the canonical one.

Public inputs = the arriving transcript (12 state words, n_in pending inputs) || per batch (the point, its opened values) || the
initial caps || the round caps || the final polynomial.  Witness inputs: the proof-of-work witness, the opened rows, the siblings, the
evaluations, the coset siblings -- every one a word of the flat proof.

Refused at build: mixed arities, salted oracles, empty batches (FriQueryRoundCircuit's refusals), pow_bits > 32, n_in > 7.
Refused at proving: Keccak Merkle trees (sipp_fri_prove_openings_h with SIPP_HASH_KECCAK25).  The opening section does not name its hasher,
so the caller does (prove_proof's `hasher`); a whole outer proof handed over in its place is read by its header word 13.  ValueError,
before anything is launched: the circuit verifies Poseidon trees only.

numpy only; imports nothing from the test oracle."""
import numpy as np

from .circuit import GEN_BASE_SPLIT, GEN_BASE_SUM, P, PUBLIC_INPUT, CircuitBuilder, CircuitProver, _Challenger, _i64, base_sum_into, pi
from .fri_verifier import GATE_NAMES as ROUND_GATE_NAMES
from .fri_verifier import POSEIDON_SWAP, FriQueryRoundCircuit, gate_groups, query_rounds_into

GATE_NAMES = ROUND_GATE_NAMES + ["BaseSplit64", "BaseSumCap", "BaseSumWithin"]
BASE_SPLIT64, BASE_SUM_CAP, BASE_SUM_WITHIN = range(len(ROUND_GATE_NAMES), len(ROUND_GATE_NAMES) + 3)
HEADER_WORDS = 8                                                # of the flat "SIPPFRI1" proof


class FriProofCircuit(FriQueryRoundCircuit):
    """FriQueryRoundCircuit's shape arguments, with pow_bits (0 .. 32), pow_rule (0, 1) and n_in, the number of input words pending in
    the arriving transcript (0 .. 7).  Cells are wire * N + row."""
    n_public_args = 6                                           # public_inputs takes partial_witness's arguments up to the final polynomial

    def __init__(self, log_m, cap_height, oracle_widths, batches, arity_bits, n_rounds, final_len, n_queries, num_wires=135, num_routed=80,
                 k_base=None, k_ext=None, min_log_n=10, pow_bits=0, pow_rule=0, n_in=0, n_salt=None):
        assert 0 <= pow_bits <= 32, "a proof of work of more than 32 bits is out of scope"
        assert pow_rule in (0, 1) and 0 <= n_in <= 7 and 65 <= num_routed
        self._set_shape(log_m, cap_height, oracle_widths, batches, arity_bits, n_rounds, final_len, n_queries, num_wires, num_routed, k_base,
                        k_ext, n_salt)
        self.pow_bits, self.pow_rule, self.n_in = pow_bits, pow_rule, n_in
        # public-input positions
        self.pi_batch, t = [], 12 + n_in
        for b in self.batches:
            self.pi_batch.append(t)
            t += 2 + 2 * len(b)
        self.pi_caps = t
        self.pi_rounds = t + 4 * self.n_cap * len(self.oracle_widths)
        self.pi_finals = self.pi_rounds + n_rounds * 4 * self.n_cap
        groups = gate_groups(cap_height, self.arity_bits)
        # the two groups of degree <= 4 are full: the BaseSum-shaped gates (degree 2) get a group of their own
        CircuitBuilder.__init__(self, num_wires, num_routed, GATE_NAMES, groups + (groups[-1] + 1,) * 3, 2, self.pi_finals + 2 * final_len)
        self._declare_proof_gates()
        self._in_keys = []
        self._wiring()
        self.finish(min_log_n)
        cells = [x for cyc in self.pi_cycle + self.in_cycle for x in cyc]
        assert len(cells) == len(set(cells))
        self._proof_layout()

    def _declare_proof_gates(self):
        """the sixteen gates of GATE_NAMES: the query rounds' thirteen, the 64-limb split and the two le_sum shapes"""
        self._declare_gates()
        self.declare(BASE_SPLIT64, 2, (GEN_BASE_SPLIT, 64, 1), base_sum_into, 64)
        self.declare(BASE_SUM_CAP, 2, (GEN_BASE_SUM, self.cap_height, 1), base_sum_into, self.cap_height)
        self.declare(BASE_SUM_WITHIN, 2, (GEN_BASE_SUM, self.arity_bits, 1), base_sum_into, self.arity_bits)
        assert _i64(1 << 63) + P == 1 << 63                     # the top limb's coefficient is a negative program word

    # public-input positions (pi_point, pi_opened, pi_cap, pi_final: the parent's, from this circuit's offsets); what is drawn in circuit
    # has none
    pi_alpha = pi_beta = pi_x_index = None

    def pi_state(self, t):
        return t

    def pi_pending(self, t):
        return 12 + t

    def pi_round_cap(self, r, j, w):
        return self.pi_rounds + 4 * (self.n_cap * r + j) + w

    def _split64(self, source):
        """the 64 one-bit limbs of a drawn value (see the module's note: not unique below 2^32 - 1, as in plonky2) -> the row"""
        r = self.new_row(BASE_SPLIT64)
        self.place(r, [(0, source)])
        return r

    def _le_sum(self, gate, bits):
        r = self.new_row(gate)
        self.place(r, [(1 + l, bit) for l, bit in enumerate(bits)])
        return r

    def _wiring(self):
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.one_row, one = self.constant(1)
        self.omega_row, omega = self.constant(self.omega_m)
        self.ginv_row, ginv = self.constant(self.g_inv)
        ch = _Challenger(self, POSEIDON_SWAP, zero, [pi(self.pi_state(t)) for t in range(12)], [pi(self.pi_pending(t)) for t in range(self.n_in)])
        self._proof_into(ch, (zero, one, omega, ginv))
        self.hash_public_inputs(POSEIDON_SWAP, zero)

    def _proof_into(self, ch, consts, opened=None, cap=None, round_cap=None, point=None, final=None):
        """The FRI transcript, the proof of work and the queries behind challenger ch (a _Challenger on this builder, with whatever it
        has absorbed so far).  consts = the cells (zero, one, omega_M, 1 / g); opened(b, j, l), cap(o, j, w), round_cap(r, j, w),
        point(b, l), final(k, l): the sources of fri_verifier.query_rounds_into, None = this circuit's public inputs.  The proof-of-work
        witness and what query_rounds_into makes are witness inputs.  Sets alpha_cells, beta_cells, response_cell, index_cells, the
        row lists, transcript_row (every row of ch so far) and transcript_levels."""
        zero = consts[0]
        opened = opened or (lambda b, j, l: pi(self.pi_opened(b, j, l)))
        round_cap = round_cap or (lambda r, j, w: pi(self.pi_round_cap(r, j, w)))
        final = final or (lambda k, l: pi(self.pi_final(k, l)))
        for b, cols in enumerate(self.batches):
            for j in range(len(cols)):
                for l in range(2):
                    ch.observe(opened(b, j, l))
        self.alpha_cells = alpha = (ch.get(), ch.get())
        self.beta_cells = []
        for r in range(self.n_rounds):
            for j in range(self.n_cap):
                for w in range(4):
                    ch.observe(round_cap(r, j, w))
            self.beta_cells.append((ch.get(), ch.get()))
        for k in range(self.final_len):
            for l in range(2):
                ch.observe(final(k, l))
        # the proof of work
        witness = self._new_input("pow_witness")
        if self.pow_rule == 0:
            ch.observe(witness)
            self.pow_hash_row, self.response_cell = [], ch.get()
        else:
            digest = [ch.get() for _ in range(4)]
            self.pow_hash_row = self.hash_rows(POSEIDON_SWAP, zero, digest + [witness])
            self.response_cell = (self.s_out, self.pow_hash_row[-1])
        self.pow_row = self._split64(self.response_cell)
        for k in range(self.pow_bits):                          # leading zeros: the top pow_bits limbs
            self.tie(zero, (64 - k, self.pow_row))
        # the queries
        self.index_cells, self.cap_sum_row, self.within_row = [], [], [[] for _ in range(self.n_queries)]

        def bits_of(q):
            self.index_cells.append(ch.get())
            bs = self._split64(self.index_cells[-1])
            return bs, [(1 + i, bs) for i in range(self.log_m)]

        def cap_index_of(q, bits):
            self.cap_sum_row.append(self._le_sum(BASE_SUM_CAP, bits))
            return (0, self.cap_sum_row[-1])

        def within_of(q, r, bits):
            self.within_row[q].append(self._le_sum(BASE_SUM_WITHIN, bits))
            return (0, self.within_row[q][-1])
        beta = self.beta_cells
        query_rounds_into(self, consts, alpha, lambda r, l: beta[r][l], bits_of, cap_index_of, within_of, opened, cap, round_cap, point, final)
        self.transcript_row = list(ch.rows)
        self.transcript_levels = max(self._level[r] for r in self.transcript_row + self.pow_hash_row) + 1

    # ---- the values ----
    def _check(self, transcript, points, opened, caps, round_caps, final_poly, pow_witness=None, queries=None):
        state, pending = transcript
        state, pending = [int(v) % P for v in state], [int(v) % P for v in pending]
        assert len(state) == 12 and len(pending) == self.n_in
        zero = (0, 0)
        head = FriQueryRoundCircuit._check(self, zero, points, opened, caps, round_caps, [zero] * self.n_rounds, final_poly, [0] * self.n_queries,
                                           queries)
        out = ((state, pending), head[1], head[2], head[3], head[4], head[6])
        if queries is None:
            return out
        return out + (int(pow_witness) % P, head[8])

    def public_inputs(self, transcript, points, opened, caps, round_caps, final_poly):
        """the arriving transcript (12 state words, the pending inputs) || per batch (point, opened values) || the initial caps || the
        round caps || the final polynomial, as ints; ext values as (c0, c1) pairs"""
        (state, pending), points, opened, caps, round_caps, final_poly = self._check(transcript, points, opened, caps, round_caps, final_poly)
        out = state + pending
        for pt, vals in zip(points, opened):
            out += list(pt) + [l for v in vals for l in v]
        for cap in caps + round_caps:
            out += [int(v) for v in cap.reshape(-1)]
        out += [l for c in final_poly for l in c]
        assert len(out) == self.n_pi
        return out

    def witness_inputs(self, *args):
        """the value of every witness input, in the order of their making"""
        pow_witness, queries = self._check(*args)[6:8]
        out = []
        for key in self._in_keys:
            kind = key[0]
            if kind == "pow_witness":
                out.append(pow_witness)
                continue
            rows, siblings, evals, coset_siblings = queries[key[1]]
            if kind == "row":
                out.append(rows[key[2]][key[3]])
            elif kind == "sibling":
                out.append(int(siblings[key[2]][key[3], key[4]]))
            elif kind == "eval":
                out.append(evals[key[2]][key[3]][key[4]])
            else:
                out.append(int(coset_siblings[key[2]][key[3], key[4]]))
        return out

    # ---- the flat proof ----
    def _proof_layout(self):
        """where every input that is a proof word sits in the flat proof: header || opened values || round caps || final polynomial ||
        the proof-of-work witness || per query (per oracle its row and siblings, per round its evaluations and coset siblings)"""
        at, pi_word = HEADER_WORDS, np.full(self.n_pi, -1, dtype=np.int64)
        for b, cols in enumerate(self.batches):
            pi_word[self.pi_opened(b, 0, 0):self.pi_opened(b, 0, 0) + 2 * len(cols)] = at + np.arange(2 * len(cols))
            at += 2 * len(cols)
        n = self.n_rounds * 4 * self.n_cap + 2 * self.final_len         # adjacent in the proof and among the public inputs
        pi_word[self.pi_rounds:self.pi_rounds + n] = at + np.arange(n)
        word = {("pow_witness",): at + n}
        at += n + 1
        for q in range(self.n_queries):
            for o, width in enumerate(self.oracle_widths):
                for k in range(width):
                    word["row", q, o, k] = at + k
                at += width
                for l in range(self.height):
                    for t in range(4):
                        word["sibling", q, o, l, t] = at + 4 * l + t
                at += 4 * self.height
            for r in range(self.n_rounds):
                for j in range(self.arity):
                    for l in range(2):
                        word["eval", q, r, j, l] = at + 2 * j + l
                at += 2 * self.arity
                for l in range(self.round_height[r]):
                    for t in range(4):
                        word["coset_sibling", q, r, l, t] = at + 4 * l + t
                at += 4 * self.round_height[r]
        self.proof_words, self.pi_word = at, pi_word
        in_word = [word[key] for key in self._in_keys]
        from_proof = np.flatnonzero(pi_word >= 0)
        cycles = [self.pi_cycle[t] for t in from_proof] + self.in_cycle
        words = [int(pi_word[t]) for t in from_proof] + in_word
        self._map = (np.array([x for cyc in cycles for x in cyc], dtype=np.uint64),
                     np.array([w for cyc, w in zip(cycles, words) for _ in cyc], dtype=np.int64))
        # the inputs that are no proof words, in public-input order: the transcript, the points (each in front of its batch's opened
        # values), the initial caps
        self.pi_other = np.flatnonzero(pi_word < 0)
        self._other = (np.array([x for t in self.pi_other for x in self.pi_cycle[t]], dtype=np.uint64),
                       np.array([k for k, t in enumerate(self.pi_other) for _ in self.pi_cycle[t]], dtype=np.int64))

    def input_map(self):
        """(cells, word_index): every cell on the cycle of a witness input, and of a public input that is a proof word, once, with the
        offset of its value in the flat proof"""
        return self._map

    def words_map(self):
        """(cells, sources, n_words, n_extra) of sipp_circuit_set_input_map: every input cell once, with the offset of its value in
        flat proof || extra, extra = the inputs that are no proof words in public-input order (transcript || points || caps)"""
        cells, word = self._map
        return (np.concatenate([cells, self._other[0]]), np.concatenate([word, self.proof_words + self._other[1]]).astype(np.uint64),
                self.proof_words, len(self.pi_other))

    def words_of_proof(self, proof, caps, points, transcript):
        """a flat proof with what it does not carry -> (words, extra, public inputs), uint64: the words are taken as they are (a
        device proof's are canonical); the public inputs are a gather from both"""
        proof = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1)
        assert len(proof) == self.proof_words
        other = np.concatenate([np.asarray(transcript[0], dtype=np.uint64).reshape(-1), np.asarray(transcript[1], dtype=np.uint64).reshape(-1),
                                np.asarray(points, dtype=np.uint64).reshape(-1), np.asarray(caps, dtype=np.uint64).reshape(-1)])
        assert len(other) == len(self.pi_other)
        pis = np.empty(self.n_pi, dtype=np.uint64)
        pis[self.pi_other] = other
        pis[self.pi_word >= 0] = proof[self.pi_word[self.pi_word >= 0]]
        return proof, other, pis

    def proof_inputs(self, proof, caps, points, transcript):
        """a flat proof with what it does not carry -> (cells, values, public inputs), uint64, by gathers alone"""
        proof, other, pis = self.words_of_proof(proof, caps, points, transcript)
        cells, word = self._map
        return np.concatenate([cells, self._other[0]]), np.concatenate([proof[word], other[self._other[1]]]), pis


def flat_proof_arguments(circ, proof, caps, points, transcript):
    """the argument tuple of FriProofCircuit.prove / partial_witness / input_cells from a flat proof, in Python integers (tests,
    tampering; FriProofProver.prove_proof does not come this way)"""
    pf, at = [int(v) for v in proof], [HEADER_WORDS]

    def take(k):
        at[0] += k
        return pf[at[0] - k:at[0]]
    pairs = lambda v: [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]
    opened = [pairs(take(2 * len(b))) for b in circ.batches]
    round_caps = [take(4 * circ.n_cap) for _ in range(circ.n_rounds)]
    final_poly = pairs(take(2 * circ.final_len))
    witness = take(1)[0]
    queries = []
    for _ in range(circ.n_queries):
        rows, sibs, evals, csibs = [], [], [], []
        for width in circ.oracle_widths:
            rows.append(take(width))
            sibs.append(take(4 * circ.height))
        for r in range(circ.n_rounds):
            evals.append(pairs(take(2 * circ.arity)))
            csibs.append(take(4 * circ.round_height[r]))
        queries.append((rows, sibs, evals, csibs))
    assert at[0] == len(pf)
    return (transcript, points, opened, caps, round_caps, final_poly, witness, queries)


class FriProofProver(CircuitProver):
    """FriProofCircuit through the library's CircuitData: built once, then prove_proof(flat proof, caps, points, transcript) or
    prove(*arguments), and verify.  prove hands the library (cell, value) pairs (sipp_circuit_prove_inputs); prove_proof hands it the
    proof's words and the device gathers them through the map set at build (sipp_circuit_prove_words), unless device_map=False keeps
    the gather in numpy."""

    def __init__(self, ctx, *shape, fri=None, params=None, digest=None, device_map=True, **kw):
        super().__init__(ctx, FriProofCircuit(*shape, **kw), fri, params, digest)
        if device_map:
            self.data.set_input_map(*self.circ.words_map())

    def prove(self, *inputs):
        c = self.circ
        cells, values = c.input_cells(*inputs)
        return self.data.prove_inputs(cells, values, c.public_inputs(*inputs[:c.n_public_args]))

    def prove_proof(self, proof, caps, points, transcript, hasher="poseidon"):
        """caps: per initial oracle 2^cap_height digests; points: per batch (c0, c1); transcript: (the 12 state words, the n_in pending
        inputs) the challenger arrives with.  No Python-integer walk of the proof, no host replay of the challenger.
        hasher: the tree hasher the opening proof was made with (the section does not name it); anything but "poseidon" is refused
        with ValueError, as is a whole outer proof whose header names Keccak."""
        from . import _lib
        if _lib.hasher_id(hasher) != _lib.HASH_POSEIDON:
            raise ValueError("FriProofProver: the circuit verifies Poseidon Merkle trees only, not hasher %r" % (hasher,))
        head = np.asarray(proof, dtype=np.uint64).reshape(-1)[:1]
        if len(head) and (int(head[0]) & 0x00ffffffffffffff) == 0x004b4c5050504953:      # "SIPPPLK?": a whole outer proof, not its opening section
            _lib.refuse_keccak_proof(proof, "FriProofProver")
        if self.data.input_map is not None:
            return self.data.prove_words(*self.circ.words_of_proof(proof, caps, points, transcript))
        return self.data.prove_inputs(*self.circ.proof_inputs(proof, caps, points, transcript))
