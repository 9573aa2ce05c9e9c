"""The whole of plonky2's verify in ONE outer circuit, for a proof of sipp_plonk_prove_gates ("SIPPPLK3"): the vanishing equation
(sipp_amd/plonk_vanishing.py's statement, _vanishing_into) and the FRI opening proof behind it (sipp_amd/fri_proof.py's, _proof_into) on
one builder, behind one challenger.  sipp_amd/plonk_vanishing.py's PlonkProofVerifier proves the same two halves as two outer proofs and
compares what they share on the host; here zeta, g zeta and the sponge state are cells that pass from one half to the other inside the
table, and the inner proof is a witness.

  PlonkVerifierCircuit   the statement "this inner proof verifies for these public inputs under this verifier data"
  flat_proof_arguments   a flat inner proof with its verifier data -> the argument tuple, in Python integers (readings, tests)
  PlonkVerifierProver    the circuit through the library's CircuitData: prove_proof(flat inner proof, constants_sigmas cap, digest)
                         sends the proof's words and lets the device gather the input cells (sipp_circuit_prove_words); verify()
                         returns the inner public inputs; with ctx = None it is the verifying half alone

Public inputs = the inner circuit digest (4) || the inner public inputs || the inner constants_sigmas cap (4 2^cap_height), hashed in
circuit (CircuitBuilder.hash_public_inputs).  Witness inputs: every other word the flat proof carries -- the wires, Z and quotient caps,
the opened values, the round caps, the final polynomial, the proof-of-work witness, per query the rows, siblings, evaluations and coset
siblings -- one witness input per word, the source of every use of it: the challenger's observation, the vanishing terms, the reduced
openings, the cap selections.

Statement.  The vanishing routine runs first; the challenger it leaves (zeta drawn last, nothing pending) goes on into the FRI
transcript.  The oracles have K + R, W, C m and C D columns; batch 0 is every column at zeta, batch 1 the C columns of Z at g zeta;
the first oracle's cap is the public constants_sigmas cap, the other three are the proof's.

Gates: sipp_amd/fri_proof.py's sixteen at their indices (the two halves' PublicInput, Constant, one-op QuotientExt and PoseidonSwap gates
are the same programs, and the vanishing half never places a BaseSum row), then the vanishing half's ArithmeticExt gate of num_routed // 8
ops and, with poseidon_mds, PoseidonMds; both join the last selector group (the three BaseSum shapes: five gates of degree <= 3).
That is 16 generators, 17 with poseidon_mds: more than the level kernels' narrow argument struct carries (include/sipp_hip.h).

Refused at build: what either half refuses -- no inner public input, more than 8 challenges, a max_degree that is no power of two, a gate
set circuit_ok refuses, poseidon_mds without an inner gate of that program, an alpha_chunk below 2; a cap height outside 1 .. 6, mixed
arities, salted (hiding) oracles, a proof of work of more than 32 bits.  Refused at proving: an inner proof whose header names Keccak Merkle
trees (header word 13, sipp_plonk_prove_gates_h): the circuit verifies Poseidon trees only -- ValueError before anything is launched.

numpy only; imports nothing from the test oracle."""
import numpy as np

from .circuit import GEN_ARITHMETIC_EXT, P, PUBLIC_INPUT, CircuitBuilder, CircuitProver, pi
from .fri_fold import EXT_W, arithmetic_ext_into
from .fri_proof import GATE_NAMES as PROOF_GATE_NAMES
from .fri_proof import HEADER_WORDS as FRI_HEADER_WORDS
from .fri_proof import FriProofCircuit
from .fri_verifier import POSEIDON_SWAP, QUOTIENT_EXT, gate_groups
from .merkle import declare_mds_gate
from .plonk_vanishing import HEADER_WORDS, MDS_IN, MDS_OUT, PlonkVanishingCircuit

ARITHMETIC_EXT_OPS = len(PROOF_GATE_NAMES)                      # the vanishing half's gate of num_routed // 8 ops
POSEIDON_MDS = ARITHMETIC_EXT_OPS + 1


class PlonkVerifierCircuit(FriProofCircuit, PlonkVanishingCircuit):
    """log_n, params (R, D, C: sipp_amd.PlonkParams or a triple), circuit (the dict of CircuitBuilder.circuit()) and n_pi_inner describe
    the INNER circuit, inner_fri (sipp_amd.FriParams, one arity for every round) its proofs.  Cells are wire * N + row."""
    n_public_args = 3                                           # public_inputs takes (digest, inner public inputs, constants_sigmas cap)
    # neither half's public-input positions exist here: every source is handed to the wiring routines
    pi_state = pi_pending = pi_point = pi_opened = pi_cap = pi_round_cap = pi_final = pi_caps = pi_zeta = None

    def __init__(self, log_n, params, circuit, inner_fri, n_pi_inner, num_wires=135, num_routed=80, min_log_n=10, poseidon_mds=False,
                 alpha_chunk=None):
        f = inner_fri
        assert 0 <= f.pow_bits <= 32, "a proof of work of more than 32 bits is out of scope"
        assert f.pow_rule in (0, 1) and 65 <= num_routed
        cap_height = min(f.cap_height, log_n + f.rate_bits)
        assert 1 <= cap_height <= 6, "a cap height outside 1 .. 6 is out of scope"
        self._set_inner(log_n, params, circuit, cap_height, n_pi_inner, num_routed, poseidon_mds, alpha_chunk)
        K, R, W, C, D, m = self.K, self.R, self.W, self.C, self.D, self.m
        arity = [int(f.arity_bits[r]) for r in range(f.n_rounds)]
        z0 = K + R + W
        self._set_shape(log_n + f.rate_bits, cap_height, [K + R, W, C * m, C * D], [list(range(self.n0)), list(range(z0, z0 + C))], arity,
                        f.n_rounds, (1 << log_n) >> sum(arity), f.num_queries, num_wires, num_routed, None, None, [4] * 4 if f.hiding else None)
        self.pow_bits, self.pow_rule, self.n_in = int(f.pow_bits), int(f.pow_rule), 0
        # public-input positions
        self.pi_digest, self.pi_inner, self.pi_cs_cap = 0, 4, 4 + n_pi_inner
        names = PROOF_GATE_NAMES + ["ArithmeticExtOps"] + (["PoseidonMds"] if self.poseidon_mds else [])
        groups = gate_groups(cap_height, self.arity_bits)
        groups += (groups[-1] + 1,) * (len(names) - len(groups))
        CircuitBuilder.__init__(self, num_wires, num_routed, names, groups, 2, self.pi_cs_cap + 4 * self.n_cap)
        self._declare_proof_gates()
        self.declare(ARITHMETIC_EXT_OPS, 3, (GEN_ARITHMETIC_EXT, self.n_ops, self.k0, self.k1, EXT_W), arithmetic_ext_into, self.n_ops, self.k0,
                     self.k1, EXT_W)
        self.mds_gate, self.swap_gate = (POSEIDON_MDS if self.poseidon_mds else None), POSEIDON_SWAP
        if self.poseidon_mds:
            declare_mds_gate(self, POSEIDON_MDS, MDS_IN, MDS_OUT)
        self._in_keys, self._word_source = [], {}
        self._wiring()
        self.finish(min_log_n)
        cells = [x for cyc in self.pi_cycle + self.in_cycle for x in cyc]
        assert len(cells) == len(set(cells))
        self._proof_layout()

    def _word(self, *key):
        """the witness input that is the proof word `key`, made at its first use: one input per word, whoever reads it"""
        if key not in self._word_source:
            self._word_source[key] = self._new_input(*key)
        return self._word_source[key]

    def _wiring(self):
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.one_row, one = self.constant(1)
        self.omega_row, omega = self.constant(self.omega_m)
        self.ginv_row, ginv = self.constant(self.g_inv)
        n_cap, n0 = self.n_cap, self.n0
        ch = self._vanishing_into((ARITHMETIC_EXT_OPS, QUOTIENT_EXT, self.mds_gate, POSEIDON_SWAP), zero, one,
                                  lambda t: pi(self.pi_digest + t), lambda t: pi(self.pi_inner + t),
                                  lambda o, t: self._word("cap", o, t), lambda k, l: self._word("opened", k, l))
        assert not ch.inbuf                                     # nothing pending: the FRI transcript's first observation discards the outputs
        # the vanishing half's challenges under names the FRI half does not take
        self.plonk_beta_cells, self.plonk_gamma_cells, self.plonk_alpha_cells = self.beta_cells, self.gamma_cells, self.alpha_cells
        self.vanishing_transcript_row, self.state_cells = list(self.transcript_row), list(ch.sponge)
        points = (self.zeta_cells, self.gzeta_cells)
        self._proof_into(ch, (zero, one, omega, ginv),
                         opened=lambda b, j, l: self._word("opened", j if b == 0 else n0 + j, l),
                         cap=lambda o, j, w: pi(self.pi_cs_cap + 4 * j + w) if o == 0 else self._word("cap", o - 1, 4 * j + w),
                         round_cap=lambda r, j, w: self._word("round_cap", r, j, w), point=lambda b, l: points[b][l],
                         final=lambda k, l: self._word("final", k, l))
        assert len(self._in_keys) == len(set(self._in_keys))
        self.hash_public_inputs(POSEIDON_SWAP, zero)

    # ---- the values ----
    def _check(self, digest, inner_pis, cs_cap, caps=None, opened=None, round_caps=None, final_poly=None, pow_witness=None, queries=None):
        digest, inner_pis, cs_cap = PlonkVanishingCircuit._check(self, digest, inner_pis, [cs_cap] * 3, [(0, 0)] * self.n_open)[:3]
        if caps is None:
            return digest, inner_pis, cs_cap[0]
        _, _, caps, opened = PlonkVanishingCircuit._check(self, digest, inner_pis, caps, opened)
        zero = (0, 0)
        head = FriProofCircuit._check(self, ([0] * 12, []), [zero, zero], [opened[:self.n0], opened[self.n0:]], [cs_cap[0]] + caps, round_caps,
                                      final_poly, pow_witness, queries)
        return digest, inner_pis, cs_cap[0], caps, opened, head[4], head[5], head[6], head[7]

    def public_inputs(self, digest, inner_pis, cs_cap):
        """the inner circuit digest || the inner public inputs || the inner constants_sigmas cap, as ints"""
        digest, inner_pis, cs_cap = self._check(digest, inner_pis, cs_cap)
        out = digest + inner_pis + [int(v) for v in cs_cap.reshape(-1)]
        assert len(out) == self.n_pi
        return out

    def witness_inputs(self, *args):
        """the value of every witness input, in the order of their making"""
        _, _, _, caps, opened, round_caps, final_poly, pow_witness, queries = self._check(*args)
        out = []
        for key in self._in_keys:
            kind = key[0]
            if kind == "cap":
                out.append(int(caps[key[1]].reshape(-1)[key[2]]))
            elif kind == "opened":
                out.append(opened[key[1]][key[2]])
            elif kind == "round_cap":
                out.append(int(round_caps[key[1]][key[2], key[3]]))
            elif kind == "final":
                out.append(final_poly[key[1]][key[2]])
            elif kind == "pow_witness":
                out.append(pow_witness)
            else:
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
        """where every input sits in flat inner proof || extra, extra = digest || constants_sigmas cap.  The proof: header (16) || the
        wires, Z and quotient caps || the opening section (its header (8), the opened values, the round caps, the final polynomial,
        the proof-of-work witness, per query per oracle the row and its siblings, per round the evaluations and coset siblings) ||
        the inner public inputs"""
        n_cap = self.n_cap
        word = {("cap", o, t): HEADER_WORDS + 4 * n_cap * o + t for o in range(3) for t in range(4 * n_cap)}
        self.section_at = HEADER_WORDS + 3 * 4 * n_cap
        at = self.section_at + FRI_HEADER_WORDS
        for k in range(self.n_open):
            for l in range(2):
                word["opened", k, l] = at + 2 * k + l
        at += 2 * self.n_open
        for r in range(self.n_rounds):
            for j in range(n_cap):
                for w in range(4):
                    word["round_cap", r, j, w] = at + 4 * (n_cap * r + j) + w
        at += self.n_rounds * 4 * n_cap
        for k in range(self.final_len):
            for l in range(2):
                word["final", k, l] = at + 2 * k + l
        at += 2 * self.final_len
        word["pow_witness",] = at
        at += 1
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
        self.proof_words, self.n_extra = at + self.n_pi_inner, 4 + 4 * n_cap
        self.word_of = word
        self.pi_word = np.concatenate([self.proof_words + np.arange(4), at + np.arange(self.n_pi_inner),
                                       self.proof_words + 4 + np.arange(4 * n_cap)]).astype(np.int64)
        cycles = self.pi_cycle + self.in_cycle
        sources = [int(w) for w in self.pi_word] + [word[key] for key in self._in_keys]
        self._map = (np.array([x for cyc in cycles for x in cyc], dtype=np.uint64),
                     np.array([s for cyc, s in zip(cycles, sources) for _ in cyc], dtype=np.uint64))

    def input_map(self, proof_words=None):
        """(cells, sources): every input cell once -- the cycles of the public inputs, then those of the witness inputs -- with the
        offset of its value in proof || extra, extra = digest || constants_sigmas cap.  The shape fixes the proof's length"""
        assert proof_words is None or proof_words == self.proof_words, "an inner proof of another length"
        return self._map

    def words_map(self):
        """(cells, sources, n_words, n_extra) of sipp_circuit_set_input_map"""
        return self._map + (self.proof_words, self.n_extra)

    proof_inputs = None                                         # the FRI circuit's numpy gather: prove_proof goes through the device map

    def words_of_proof(self, proof, cs_cap, digest):
        """a flat inner proof with its verifier data -> (words, extra, public inputs), uint64: one concatenate, one gather"""
        proof = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1)
        assert len(proof) == self.proof_words, "an inner proof of another length"
        extra = np.concatenate([np.array([int(v) % P for v in digest], dtype=np.uint64), np.asarray(cs_cap, dtype=np.uint64).reshape(-1)])
        assert len(extra) == self.n_extra
        return proof, extra, np.concatenate([proof, extra])[self.pi_word]


def flat_proof_arguments(circ, proof, cap, digest):
    """the argument tuple of PlonkVerifierCircuit.public_inputs (its first three) / partial_witness / input_cells and of
    PlonkVerifierProver.prove from a flat inner proof, its circuit's constants_sigmas cap and digest, in Python integers"""
    from .fri_proof import flat_proof_arguments as fri_arguments
    pf, n_cap = [int(v) for v in proof], circ.n_cap
    assert len(pf) == circ.proof_words
    caps = [np.array(pf[HEADER_WORDS + 4 * n_cap * o:HEADER_WORDS + 4 * n_cap * (o + 1)], dtype=np.uint64).reshape(n_cap, 4) for o in range(3)]
    cs_cap = np.asarray(cap, dtype=np.uint64).reshape(n_cap, 4)
    _, _, opened, _, round_caps, final_poly, witness, queries = fri_arguments(circ, pf[circ.section_at:len(pf) - circ.n_pi_inner], None, None, None)
    return (list(digest), pf[len(pf) - circ.n_pi_inner:], cs_cap, caps, opened[0] + opened[1], round_caps, final_poly, witness, queries)


class PlonkVerifierProver(CircuitProver):
    """PlonkVerifierCircuit through the library's CircuitData: built once (shape = the circuit's arguments), then prove_proof / prove /
    verify.  ctx = None builds the verifying half alone, without a device: verifier_data = this OUTER circuit's (constants_sigmas cap,
    digest), fri and params as the prover had them."""

    def __init__(self, ctx, *shape, fri=None, params=None, digest=None, verifier_data=None, **kw):
        from . import _lib
        if ctx is None:
            assert verifier_data is not None and fri is not None
            self.circ, self.data, self.fri = PlonkVerifierCircuit(*shape, **kw), None, fri
            self.params = params if params is not None else _lib.PlonkParams(self.circ.num_routed, 8, 2)
            self.circuit = self.circ.circuit()
            self._pc = _lib.PlonkCircuit.from_dict(self.circuit)
            self.cap = np.ascontiguousarray(verifier_data[0], dtype=np.uint64).reshape(-1, 4)
            self.digest = np.array([int(x) for x in verifier_data[1]], dtype=np.uint64)
        else:
            super().__init__(ctx, PlonkVerifierCircuit(*shape, **kw), fri, params, digest)
        self._mapped = False

    def prove(self, *inputs):
        c = self.circ
        cells, values = c.input_cells(*inputs)
        return self.data.prove_inputs(cells, values, c.public_inputs(*inputs[:c.n_public_args]))

    def prove_proof(self, inner_proof, constants_sigmas_cap, digest):
        """the outer proof of one flat inner proof: the map from its words to the input cells goes to the device once"""
        from ._lib import refuse_keccak_proof
        refuse_keccak_proof(inner_proof, "PlonkVerifierProver")
        c = self.circ
        words, extra, pis = c.words_of_proof(inner_proof, constants_sigmas_cap, digest)
        if not self._mapped:
            self.data.set_input_map(*c.words_map())
            self._mapped = True
        return self.data.prove_words(words, extra, pis)

    def _verdict(self, proof):
        """sipp_plonk_verify_gates (host code) with this outer circuit's verifier data -> (status, refusing stage)"""
        import ctypes as C
        from . import _lib
        pf = np.ascontiguousarray(proof, dtype=np.uint64)
        cap, dg = np.ascontiguousarray(self.cap, dtype=np.uint64).reshape(-1), np.ascontiguousarray(self.digest, dtype=np.uint64)
        reason, u64p = C.c_int(0), C.POINTER(C.c_uint64)
        rc = _lib.lib().sipp_plonk_verify_gates(pf.ctypes.data_as(u64p), len(pf), cap.ctypes.data_as(u64p), C.byref(self.params), C.byref(self.fri),
                                                C.byref(self._pc), dg.ctypes.data_as(u64p), C.byref(reason))
        return rc, reason.value

    def verify(self, proof, constants_sigmas_cap=None, digest=None):
        """verify(proof) -> (status, refusing stage) of the outer proof alone, as every CircuitProver; verify(proof, the inner
        circuit's constants_sigmas cap, its digest) -> the inner public inputs, or ValueError naming what refuses"""
        if constants_sigmas_cap is None and digest is None:
            return self._verdict(proof)
        c = self.circ
        if len(proof) < c.n_pi:
            raise ValueError("the proof is too short")
        verdict = self._verdict(proof)
        if verdict != (0, 0):
            raise ValueError("the proof is refused: status %d at stage %d" % tuple(verdict))
        pis = [int(x) for x in proof[len(proof) - c.n_pi:]]
        if pis[c.pi_cs_cap:] != [int(x) for x in np.asarray(constants_sigmas_cap, dtype=np.uint64).reshape(-1)]:
            raise ValueError("the proof verifies under another constants_sigmas cap")
        if pis[c.pi_digest:c.pi_digest + 4] != [int(x) % P for x in digest]:
            raise ValueError("the proof is for another circuit digest")
        return pis[c.pi_inner:c.pi_inner + c.n_pi_inner]

    def close(self):
        if self.data is not None:
            self.data.close()
