"""SIPP's Fiat-Shamir transcript in the outer circuit: what the reference's sipp_verifier_circuit does besides verifying the three STARK
proofs (reference src/transcript_circuit.rs, src/verifier_circuit.rs).  The transcript is a Poseidon hash chain over A, B, Z and every
round's Z_L / Z_R; each round hashes the state once more, reads the four digest words as eight u32 limbs, reduces them modulo the BN254
scalar prime r to the challenge x and inverts x; x and x^-1 are the exp_val of every G1 / G2 / Fq12 obligation of that round.

  TranscriptGadget          the reference's names on a builder: append, append_g1, append_g2, append_fq12, get_challenge
  SippTranscriptCircuit     the statement for n pairs (a power of two, n >= 2)
  SippTranscriptProver      the circuit through the library's CircuitData: prove, prove_words, challenges_of, check_obligations

state <- hash_no_pad(state || msg) is a chain of swap-0 Poseidon rows (CircuitBuilder.hash_rows); get_challenge hashes the state once
more and sends each digest word through a 64-limb split (one-bit limbs) and two 32-bit le_sums.
The 64-bit split of a field element is not unique: a value v < 2^32 - 1 is also the limbs of v + p.  plonky2's recursive verifier
accepts that (split_le of a challenge, fri/recursive_verifier.rs), and so does this circuit: a prover may take either reading of such
a digest word, one chance in 2^32 per word.  The generator writes the canonical one.
reduce and inverse are sipp_amd/nonnative.py's: the challenge and its inverse are THE values the native verifier computes.

Public inputs = A (16 n) || B (32 n) || Z (96) || per round x (8) || x^-1 (8).  The x / x^-1 cells are generated: the public inputs
are tied to them, and the chain that hashes the public inputs reads them from the cells that hold them.  Witness inputs: Z_L (96) ||
Z_R (96) of every round, in round order, and nothing else; quotients, remainders, inverses, bits and carries are all generated.

NOT checked in circuit: that the statement and Z_L / Z_R words are u32 -- they are hashed as given, and the STARK proofs' public inputs
carry the same words; anything about the STARK proofs.
Divergence from the NATIVE transcript (documented, not fixed): the native get_challenge reads the digest through BigUint::to_u32_digits,
which drops a zero high half; this circuit, like the reference's circuit, always takes eight limbs.  The two differ only
when a digest word is below 2^32 or is zero.

numpy only; imports nothing from the test oracle."""
import numpy as np

from .circuit import BASE_SUM, GEN_BASE_SUM, P, PUBLIC_INPUT, CircuitProver, base_sum_into, pi
from .merkle import declare_swap_gate
from .nonnative import NonnativeBuilder

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # the BN254 scalar prime
GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSplit64", "LeSum32", "NonnativeInverse", "U32Range", "U32Arithmetic", "U32AddMany",
              "NonnativeReduce", "PoseidonSwap"]
GATE_GROUP = (0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2)                  # degree 2 with five others; degree 4 in a group of four; degree 7 alone
LE_SUM32, NN_INVERSE, U32_RANGE, U32_ARITH, U32_ADD, NN_REDUCE, POSEIDON_SWAP = range(4, 11)
M32 = 0xFFFFFFFF


class TranscriptGadget:
    """reference src/transcript_circuit.rs on a builder: sources in, cells out"""

    def __init__(self, b, gate, zero):
        self.b, self.gate, self.zero, self.state, self.rows = b, gate, zero, [zero] * 4, []

    def append(self, msg):
        rows = self.b.hash_rows(self.gate, self.zero, self.state + list(msg))
        self.state = [(self.b.s_out + t, rows[-1]) for t in range(4)]
        self.rows += rows

    def append_g1(self, words):
        assert len(words) == 16
        self.append(words)

    def append_g2(self, words):
        assert len(words) == 32
        self.append(words)

    def append_fq12(self, words):
        assert len(words) == 96
        self.append(words)

    def get_challenge(self):
        """hash_no_pad(state) as eight u32 limb cells (the state stays); -> (the limbs, the split rows)"""
        b = self.b
        rows = b.hash_rows(self.gate, self.zero, self.state)
        self.rows += rows
        limbs, splits = [], []
        for t in range(4):
            sp = b.new_row(BASE_SUM)
            b.place(sp, [(0, (b.s_out + t, rows[-1]))])
            splits.append(sp)
            for half in range(2):
                r = b.new_row(LE_SUM32)
                b.place(r, [(1 + l, (1 + 32 * half + l, sp)) for l in range(32)])
                limbs.append((0, r))
        return limbs, splits


class SippTranscriptCircuit(NonnativeBuilder):
    """The transcript of a SIPP proof over n pairs.  Cells are wire * N + row."""
    n_public_args = 3

    def __init__(self, n, num_wires=135, num_routed=80, min_log_n=10):
        if not (isinstance(n, int) and n >= 2 and n & (n - 1) == 0):
            raise ValueError("SippTranscriptCircuit: n must be a power of two, at least 2 (got %r)" % (n,))
        assert num_wires >= 135 and num_routed >= 65
        self.n_pairs, self.rounds = n, n.bit_length() - 1
        self.n_statement = 48 * n + 96
        self.n_round_words = 192 * self.rounds
        super().__init__(num_wires, num_routed, GATE_NAMES, GATE_GROUP, 1, self.n_statement + 16 * self.rounds)
        self.declare_basic(64)                                  # BaseSum: the 64-limb split
        self.declare(LE_SUM32, 2, (GEN_BASE_SUM, 32, 1), base_sum_into, 32)
        self.declare_nonnative(U32_RANGE, U32_ARITH, U32_ADD, NN_REDUCE, NN_INVERSE)
        declare_swap_gate(self, POSEIDON_SWAP)
        self._wiring()
        self.finish(min_log_n)
        cells = [x for cyc in self.pi_cycle + self.in_cycle for x in cyc]
        assert len(cells) == len(set(cells))
        # the map of prove_words: words = statement || round words, extra = the claimed challenges
        cs, ss = [], []
        for t, cyc in enumerate(self.pi_cycle):
            cs += cyc
            ss += [t if t < self.n_statement else self.n_statement + self.n_round_words + (t - self.n_statement)] * len(cyc)
        for k, cyc in enumerate(self.in_cycle):
            cs += cyc
            ss += [self.n_statement + k] * len(cyc)
        self._map = (np.array(cs, dtype=np.uint64), np.array(ss, dtype=np.uint64))

    def _wiring(self):
        n = self.n_pairs
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.one_row, one = self.constant(1)
        self.set_constants(zero, one)
        self.modulus_cells = [self.constant((R >> (32 * k)) & M32)[1] for k in range(8)]
        t = TranscriptGadget(self, POSEIDON_SWAP, zero)
        for i in range(n):
            t.append_g1([pi(16 * i + w) for w in range(16)])
            t.append_g2([pi(16 * n + 32 * i + w) for w in range(32)])
        t.append_fq12([pi(48 * n + w) for w in range(96)])
        self.round_inputs, self.digest_limbs, self.split_rows, self.x_cells, self.xinv_cells = [], [], [], [], []
        for _ in range(self.rounds):
            words = [self.witness_input() for _ in range(192)]
            self.round_inputs.append(words)
            t.append_fq12(words[:96])
            t.append_fq12(words[96:])
            limbs, splits = t.get_challenge()
            x = self.reduce(limbs, self.modulus_cells)
            self.digest_limbs.append(limbs)
            self.split_rows.append(splits)
            self.x_cells.append(x)
            self.xinv_cells.append(self.inverse(x, self.modulus_cells))
        self.transcript_rows = t.rows
        # the outputs, public: the chain that hashes the public inputs reads them from the cells that hold them
        outs = [c for k in range(self.rounds) for c in self.x_cells[k] + self.xinv_cells[k]]
        self.chain_row = self.hash_rows(POSEIDON_SWAP, zero, [pi(w) for w in range(self.n_statement)] + outs)
        for k, s in enumerate(outs):
            self.public_input(self.n_statement + k, s)
        for w in range(4):
            self.tie((self.s_out + w, self.chain_row[-1]), (w, self.pi_row))

    # ---- inputs ----
    def _check(self, statement_words, round_words, challenges):
        st = [int(v) % P for v in np.asarray(statement_words).reshape(-1)]
        rw = [int(v) % P for v in np.asarray(round_words).reshape(-1)]
        ch = [int(v) % P for v in np.asarray(challenges).reshape(-1)]
        assert len(st) == self.n_statement and len(rw) == self.n_round_words and len(ch) == 16 * self.rounds
        return st, rw, ch

    def public_inputs(self, statement_words, round_words, challenges):
        """A || B || Z || per round x (8 limbs) || x^-1 (8 limbs), as ints (the round words are not public)"""
        st, _, ch = self._check(statement_words, round_words, challenges)
        return st + ch

    def input_cells(self, statement_words, round_words, challenges):
        """(cells, values) of sipp_circuit_prove_inputs: every cell on a cycle of a public input or of a witness input"""
        st, rw, ch = self._check(statement_words, round_words, challenges)
        words = np.array(st + rw + ch, dtype=np.uint64)
        return self._map[0], words[self._map[1].astype(np.int64)]

    def partial_witness(self, statement_words, round_words, challenges):
        """[num_wires][N] with the input cells set, everything else 0"""
        cells, values = self.input_cells(statement_words, round_words, challenges)
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        w.reshape(-1)[cells.astype(np.int64)] = values
        return w

    def words_map(self):
        """(cells, sources, n_words, n_extra) of sipp_circuit_set_input_map: words = statement || round words, extra = the challenges"""
        return self._map + (self.n_statement + self.n_round_words, 16 * self.rounds)


def challenges_of(fq12_records):
    """the exponents of an obligation list (verify_native's Fq12 records, [2 rounds][296] u32: x at 192 .. 200 of record 2 k, x^-1 of
    record 2 k + 1) -> per round x (8) || x^-1 (8), flat"""
    fq = np.asarray(fq12_records, dtype=np.uint64).reshape(-1, 296)
    assert len(fq) >= 2 and len(fq) % 2 == 0
    return [int(v) for k in range(len(fq) // 2) for v in list(fq[2 * k, 192:200]) + list(fq[2 * k + 1, 192:200])]


def check_obligations(c, public_inputs, g1, g2, fq12):
    """whether every record's exp_val is its round's x (G1, the first Fq12 record of the round) or x^-1 (G2, the second): the G1 /
    G2 lists hold n / 2, n / 4, .. 1 records round by round, exponents at 32 .. 40 of 56 and at 64 .. 72 of 104"""
    pis = [int(v) for v in public_inputs]
    g1 = np.asarray(g1, dtype=np.uint64).reshape(-1, 56)
    g2 = np.asarray(g2, dtype=np.uint64).reshape(-1, 104)
    fq = np.asarray(fq12, dtype=np.uint64).reshape(-1, 296)
    if len(pis) != c.n_pi or len(g1) != c.n_pairs - 1 or len(g2) != c.n_pairs - 1 or len(fq) != 2 * c.rounds:
        return False
    at, ok = 0, True
    for k in range(c.rounds):
        x = pis[c.n_statement + 16 * k:c.n_statement + 16 * k + 8]
        xi = pis[c.n_statement + 16 * k + 8:c.n_statement + 16 * k + 16]
        for _ in range(c.n_pairs >> (k + 1)):
            ok &= [int(v) for v in g1[at, 32:40]] == x and [int(v) for v in g2[at, 64:72]] == xi
            at += 1
        ok &= [int(v) for v in fq[2 * k, 192:200]] == x and [int(v) for v in fq[2 * k + 1, 192:200]] == xi
    return bool(ok)


class SippTranscriptProver(CircuitProver):
    """SippTranscriptCircuit through the library's CircuitData: built once, the input map fixed at build"""

    def __init__(self, ctx, n, fri=None, params=None, digest=None, min_log_n=10):
        super().__init__(ctx, SippTranscriptCircuit(n, min_log_n=min_log_n), fri, params, digest)
        self.data.set_input_map(*self.circ.words_map())

    def prove(self, statement_words, round_words, challenges):
        """through sipp_circuit_prove_inputs"""
        c = self.circ
        cells, values = c.input_cells(statement_words, round_words, challenges)
        return self.data.prove_inputs(cells, values, c.public_inputs(statement_words, round_words, challenges))

    def prove_words(self, statement_words, round_words, challenges):
        """through sipp_circuit_prove_words: the same bytes as prove()"""
        st, rw, ch = self.circ._check(statement_words, round_words, challenges)
        return self.data.prove_words(np.array(st + rw, dtype=np.uint64), np.array(ch, dtype=np.uint64), np.array(st + ch, dtype=np.uint64))

    challenges_of = staticmethod(challenges_of)

    def check_obligations(self, public_inputs, g1, g2, fq12):
        """check_obligations() of this module for the prover's circuit"""
        return check_obligations(self.circ, public_inputs, g1, g2, fq12)
