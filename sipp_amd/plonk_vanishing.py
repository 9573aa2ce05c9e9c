"""The first half of plonky2's verify in the outer circuit, for a proof of sipp_plonk_prove_gates ("SIPPPLK3"): everything plonk_verify
(sipp_amd/csrc/verify.cpp) does before it hands over to the FRI verifier, restated on cells.  beta, gamma, alpha and zeta are drawn IN
CIRCUIT from the circuit digest, the public-input hash and the three caps; the permutation argument and the inner circuit's gate
constraints are evaluated at zeta from the opened values; the result is tied to Z_H(zeta) times the quotient chunks.

  PlonkVanishingCircuit   the statement "these opened values meet the vanishing equation behind this transcript"; zeta, g zeta and the
                          departing sponge state are public OUTPUTS, for sipp_amd/fri_proof.py's circuit to take over from
  PlonkVanishingProver    the circuit through the library's CircuitData: prove_proof(flat inner proof, digest)
  _vanishing_into         (a method of the circuit) the statement as a routine over sources: this circuit passes its public inputs,
                          sipp_amd/plonk_verifier.py's joined circuit its witness inputs, and goes on with the challenger it returns

The gate compiler.  The inner gate set is data: per gate a selector and one polynomial per constraint as monomials (the program words
verify.cpp and circuit_ok read: a monomial count per constraint, per monomial an int64 coefficient -- negative words mean p + c -- and
(kind, index) factor pairs, kind 0 an opened wire, 1 an opened constant, 2 a word of the public-input hash).  The compiler turns that
data into ArithmeticExtension ops  out = c0 a m + c1 c  (c0, c1 the row's constants).  A monomial is its sorted factor list; every
distinct one is evaluated once: the product of a list is the product of the list without its last factor times that factor, so powers
of one operand chain and lists share every prefix already built.  A constraint accumulates  coefficient value one + acc; term j is the
sum over the gates of filter_g constraint_(g, j), filter_g = prod over the group's other gates i of (i - s), times (0xFFFFFFFF - s)
when there is more than one selector column.

Rows.  An op is written down when it is asked for and placed later (_Ops.flush): ops whose operands are all placed go first, then
those that read them, and so on; within one such round ops with equal (c0, c1) share rows, num_routed // 8 to a row.  place() derives
every level from the sources.

The Poseidon gate through MDS rows (poseidon_mds=True).  The inner gate whose program words are merkle.poseidon_swap_gate() at
SWAP_LAYOUT is not compiled from its 5365 monomials: its 123 constraint values, the same field elements in the same order, come from
walking the permutation on the opened wires (_poseidon_constraints), the linear layers as rows of a PoseidonMds gate (plonky2's
PoseidonMdsGate; SIPP_GEN_POSEIDON_MDS) that joins the two extension gates' selector group: 30 rows, of which only the 22 partial
rounds' chain.  alpha_chunk=K cuts the closing Horner in alpha, the longest chain left, into chunks of K terms and runs Horner in
alpha^K over the chunk sums.  Both are part of the circuit's shape; the defaults build the circuit that was built without them.

Public inputs = the inner circuit digest (4) || the inner public inputs || the wires, Z and quotient caps || the opened values in the
proof's order (constants, sigmas, wires, Z and partial products, quotient chunks, then Z at g zeta), each (c0, c1) || zeta (2) ||
g zeta (2) || the departing sponge state (12).  The last 16 are generated cells: the partial witness does not set them, the prover
passes their values (transcript(), by the library's host permutation) as public inputs.

Refused at build: no inner public input, more than 8 challenges, a max_degree that is no power of two, a gate set circuit_ok refuses,
poseidon_mds without an inner gate of exactly that program, an alpha_chunk below 2.  Refused at proving (ValueError, nothing launched): an
inner proof whose header word 13 names Keccak Merkle trees -- its caps are then 25-byte digests the Poseidon-only FRI half cannot check.

numpy only; imports nothing from the test oracle."""
import numpy as np

from .circuit import (GEN_ARITHMETIC_EXT, GEN_QUOTIENT_EXT, P, PUBLIC_INPUT, SWAP_LAYOUT, UNUSED, CircuitBuilder, CircuitProver, _Challenger,
                      _root_of_unity, pi)
from .fri_fold import EXT_W, arithmetic_ext_into
from .merkle import declare_mds_gate, declare_swap_gate, poseidon_swap_gate, poseidon_tables, sbox_wire

GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "ArithmeticExt", "QuotientExt", "PoseidonSwap"]
GATE_GROUP = (0, 0, 0, 0, 1, 1, 2)
ARITHMETIC_EXT, QUOTIENT_EXT, POSEIDON_SWAP = 4, 5, 6
# with poseidon_mds the gate set gains PoseidonMds in the group of the two extension gates; PoseidonSwap moves up by one
MDS_GATE_NAMES = GATE_NAMES[:6] + ["PoseidonMds", "PoseidonSwap"]
MDS_GATE_GROUP = (0, 0, 0, 0, 1, 1, 1, 2)
POSEIDON_MDS = 6
MDS_IN, MDS_OUT = 0, 24                                         # the MDS rows' layout: 24 cells in, 24 cells out, all routed
HEADER_WORDS, FRI_HEADER_WORDS = 16, 8                          # of the flat "SIPPPLK3" proof and of its opening section


def circuit_ok(circ, num_routed):
    """verify.cpp's circuit_ok over the circuit dict -> None, or what is wrong"""
    W, K, S, gates = circ["num_wires"], circ["num_constants"], circ["num_selectors"], circ["gates"]
    prog = [int(x) for x in circ["programs"]]
    if W < num_routed or S == 0 or S > K or not gates:
        return "shape"
    for sel, row, lo, hi, off, ncons in gates:
        if sel >= S or lo > row or row >= hi or hi > len(gates):
            return "a gate outside its group"
        w = off
        for _ in range(ncons):
            if w >= len(prog):
                return "a program behind the words"
            nm, w = prog[w], w + 1
            if nm < 0 or nm > 4096:
                return "a monomial count out of range"
            for _ in range(nm):
                if w + 2 > len(prog):
                    return "a program behind the words"
                nf, w = prog[w + 1], w + 2
                if nf < 0 or nf > 64 or w + 2 * nf > len(prog):
                    return "a factor count out of range"
                for _ in range(nf):
                    kind, idx = prog[w], prog[w + 1]
                    w += 2
                    if kind < 0 or kind > 2 or idx < 0 or (kind == 0 and idx >= W) or (kind == 1 and idx >= K) or (kind == 2 and idx >= 4):
                        return "a factor out of range"
    return None


def gate_constraints(circ, gate):
    """the program words of one gate -> per constraint [(coefficient mod p, the sorted factor tuple)]"""
    prog, (_, _, _, _, w, ncons) = circ["programs"], circ["gates"][gate]
    out = []
    for _ in range(ncons):
        nm, w = int(prog[w]), w + 1
        monos = []
        for _ in range(nm):
            coef, nf = int(prog[w]) % P, int(prog[w + 1])
            w += 2
            monos.append((coef, tuple(sorted((int(prog[w + 2 * f]), int(prog[w + 2 * f + 1])) for f in range(nf)))))
            w += 2 * nf
        out.append(monos)
    return out


def gate_words(circ, gate):
    """the program words of one gate, by walking them (circuit_ok has accepted the circuit)"""
    prog, (_, _, _, _, off, ncons) = circ["programs"], circ["gates"][gate]
    w = off
    for _ in range(ncons):
        nm, w = int(prog[w]), w + 1
        for _ in range(nm):
            w += 2 + 2 * int(prog[w + 1])
    return np.asarray(prog[off:w], dtype=np.int64)


class _V:
    """an extension value: a pair of sources once it is placed (src), the op that makes it until then (an ArithmeticExtension op's
    tuple, or ("mds", row) for an output of a PoseidonMds row)"""
    __slots__ = ("src", "op", "depth")

    def __init__(self, src=None, op=None, depth=0):
        self.src, self.op, self.depth = src, op, depth


class _Mds:
    """a PoseidonMds row until it is placed: twelve values in, twelve out"""
    __slots__ = ("ins", "outs", "depth")

    def __init__(self, ins):
        self.ins, self.outs, self.depth = list(ins), [], 0


class _Ops:
    """ArithmeticExtension ops of a builder, written down first and placed in rounds (the module's note on rows); with mds_gate also
    PoseidonMds rows, each a row of its own one round behind its latest operand"""

    SLACK = 0                                                   # rounds an op may wait for a row of its constants: 0 keeps every op at its depth

    def __init__(self, b, gate, n_ops, mds_gate=None):
        self.b, self.gate, self.n_ops, self.pending, self.rows, self.count = b, gate, n_ops, [], [], 0
        self.mds_gate, self.mds_rows, self.made = mds_gate, [], 0

    def op(self, c0, c1, a, m, c=None):
        """c0 a m + c1 c"""
        v = _V(op=(c0 % P, c1 % P, a, m, c))
        self.pending.append(v)
        self.made += 1
        return v

    def mds(self, ins):
        """M ins, element by element: the twelve outputs of a PoseidonMds row"""
        row = _Mds(ins)
        assert self.mds_gate is not None and len(row.ins) == 12
        row.outs = [_V(op=("mds", row)) for _ in range(12)]
        self.pending.append(row)
        return list(row.outs)

    def flush(self):
        """rounds: an op goes behind its operands, and into a row of its constants that still has room there or later (within SLACK
        rounds: waiting packs the rows, and delays only what reads the op), else into a new row at its earliest round"""
        b, rounds, open_rows = self.b, {}, {}
        for v in self.pending:                                  # in the order of their making: operands first
            if isinstance(v, _Mds):
                v.depth = 1 + max((x.depth for x in v.ins if x.op is not None), default=0)
                for o in v.outs:
                    o.depth = v.depth
                rounds.setdefault(v.depth, []).append(v)
                continue
            first = 1 + max((x.depth for x in v.op[2:] if x is not None and x.op is not None), default=0)
            slots = open_rows.setdefault(v.op[:2], {})
            at = min((r for r, row in slots.items() if first <= r <= first + self.SLACK and len(row) < self.n_ops), default=None)
            if at is None:
                at = first
                slots[at] = []
                rounds.setdefault(at, []).append(slots[at])
            slots[at].append(v)
            v.depth = at
        for at in sorted(rounds):
            for vs in rounds[at]:
                if isinstance(vs, _Mds):
                    r = b.new_row(self.mds_gate)
                    b.place(r, [(MDS_IN + 2 * k + l, x.src[l]) for k, x in enumerate(vs.ins) for l in range(2)])
                    for k, o in enumerate(vs.outs):
                        o.src = ((MDS_OUT + 2 * k, r), (MDS_OUT + 2 * k + 1, r))
                    self.mds_rows.append(r)
                    continue
                c0, c1 = vs[0].op[:2]
                r = b.new_row(self.gate, c0, c1)
                feeds = []
                for k, v in enumerate(vs):
                    for i, x in enumerate(v.op[2:]):
                        if x is not None:
                            feeds += [(8 * k + 2 * i, x.src[0]), (8 * k + 2 * i + 1, x.src[1])]
                b.place(r, feeds)
                for k, v in enumerate(vs):
                    v.src = ((8 * k + 6, r), (8 * k + 7, r))
                self.rows.append(r)
                self.count += len(vs)
        for v in self.pending:                                  # placed: leaves of whatever comes next
            for x in (v.outs if isinstance(v, _Mds) else (v,)):
                x.op, x.depth = None, 0
        self.pending = []


class _HostChallenger:
    """host::Challenger over the library's host permutation (sipp_host_poseidon_permute): what the circuit's transcript must draw"""

    def __init__(self):
        self.state, self.inbuf, self.outbuf = [0] * 12, [], []

    def _duplex(self):
        from . import _lib
        self.state[:len(self.inbuf)] = self.inbuf
        st = np.array(self.state, dtype=np.uint64)
        rc = _lib.lib().sipp_host_poseidon_permute(st.ctypes.data, 1, -1)
        assert rc == 0
        self.state = [int(v) for v in st]
        self.inbuf, self.outbuf = [], self.state[:8]

    def observe(self, v):
        self.outbuf = []
        self.inbuf.append(int(v) % P)
        if len(self.inbuf) == 8:
            self._duplex()

    def get(self):
        if self.inbuf or not self.outbuf:
            self._duplex()
        return self.outbuf.pop()

    def hash_no_pad(self, words):
        """hash_n_to_hash_no_pad, overwrite mode"""
        h = _HostChallenger()
        for at in range(0, len(words), 8):
            h.inbuf = [int(v) % P for v in words[at:at + 8]]
            h._duplex()
        return h.state[:4]


class PlonkVanishingCircuit(CircuitBuilder):
    """log_n, params (num_routed_wires R, max_degree D, num_challenges C: sipp_amd.PlonkParams or a triple), circuit (the dict of
    CircuitBuilder.circuit()) and n_pi_inner describe the INNER circuit; cap_height is its proofs'.  Cells are wire * N + row."""
    n_public_args = 4

    def __init__(self, log_n, params, circuit, cap_height, n_pi_inner, num_wires=135, num_routed=80, min_log_n=10, poseidon_mds=False,
                 alpha_chunk=None):
        """poseidon_mds: the inner gate whose program is merkle.poseidon_swap_gate() at SWAP_LAYOUT, word for word, is evaluated
        numerically through PoseidonMds rows (_poseidon_constraints) instead of from its monomials; refused if there is none.
        alpha_chunk = K >= 2: the closing Horner in alpha runs inside chunks of K terms, then in alpha^K over the chunk sums"""
        self._set_inner(log_n, params, circuit, cap_height, n_pi_inner, num_routed, poseidon_mds, alpha_chunk)
        # public-input positions
        self.pi_digest, self.pi_inner = 0, 4
        self.pi_caps = 4 + n_pi_inner
        self.pi_opened = self.pi_caps + 3 * 4 * self.n_cap
        self.pi_zeta = self.pi_opened + 2 * self.n_open
        self.pi_gzeta, self.pi_state = self.pi_zeta + 2, self.pi_zeta + 4
        self.mds_gate, self.swap_gate = (POSEIDON_MDS, POSEIDON_MDS + 1) if self.poseidon_mds else (None, POSEIDON_SWAP)
        names, group = (MDS_GATE_NAMES, MDS_GATE_GROUP) if self.poseidon_mds else (GATE_NAMES, GATE_GROUP)
        CircuitBuilder.__init__(self, num_wires, num_routed, names, group, 2, self.pi_state + 12)
        self.declare_basic(1)
        self.declare(ARITHMETIC_EXT, 3, (GEN_ARITHMETIC_EXT, self.n_ops, self.k0, self.k1, EXT_W), arithmetic_ext_into, self.n_ops, self.k0,
                     self.k1, EXT_W)
        self.declare(QUOTIENT_EXT, 3, (GEN_QUOTIENT_EXT, 1, self.k0, self.k1, EXT_W), arithmetic_ext_into, 1, self.k0, self.k1, EXT_W)
        if self.poseidon_mds:
            declare_mds_gate(self, self.mds_gate, MDS_IN, MDS_OUT)
        declare_swap_gate(self, self.swap_gate)
        self._wiring()
        self.finish(min_log_n)

    def _set_inner(self, log_n, params, circuit, cap_height, n_pi_inner, num_routed, poseidon_mds, alpha_chunk):
        """the inner circuit's shape with its refusals, and what the statement (_vanishing_into) reads of it; sipp_amd/plonk_verifier.py's
        circuit takes the same"""
        assert alpha_chunk is None or (isinstance(alpha_chunk, int) and alpha_chunk >= 2), "alpha_chunk must be an int of at least 2"
        self.poseidon_mds, self.alpha_chunk = bool(poseidon_mds), alpha_chunk
        R, D, C = ((params.num_routed_wires, params.max_degree, params.num_challenges) if hasattr(params, "max_degree") else
                   tuple(int(x) for x in params))
        assert n_pi_inner > 0, "an inner proof without public inputs has no public-input hash to build"
        assert 1 <= C <= 8, "more than 8 challenges are out of scope"
        assert 2 <= D <= 64 and D & (D - 1) == 0, "max_degree must be a power of two (2 .. 64)"
        assert R >= 1 and 1 <= log_n <= 26 and 0 <= cap_height <= 16
        assert not any(circuit.get("lookup", ())), "an inner circuit with lookups (a \"SIPPPLK4\" proof) is out of scope"
        bad = circuit_ok(circuit, R)
        assert bad is None, "the inner gate set is refused: %s" % bad
        self.inner_log_n, self.R, self.D, self.C, self.inner, self.inner_cap_height, self.n_pi_inner = log_n, R, D, C, circuit, cap_height, n_pi_inner
        self.W, self.K = circuit["num_wires"], circuit["num_constants"]
        self.m = -(-R // D)
        self.np_ = self.m - 1
        self.nz = C * self.m
        self.n0 = self.K + R + self.W + self.nz + C * D
        self.n_open = self.n0 + C
        self.n_cap = 1 << cap_height
        self.ngc = max(g[5] for g in circuit["gates"])
        self.n_ops = num_routed // 8
        assert self.n_ops >= 1 and 25 <= num_routed
        self.routed_gates = []
        if self.poseidon_mds:
            want = poseidon_swap_gate(**SWAP_LAYOUT)
            self.routed_gates = [g for g, gate in enumerate(circuit["gates"]) if gate[5] == 123 and np.array_equal(gate_words(circuit, g), want)]
            assert self.routed_gates, "poseidon_mds: no inner gate's program is the Poseidon swap gate's at SWAP_LAYOUT"
            assert MDS_OUT + 24 <= num_routed

    # ---- the statement ----
    def _wiring(self):
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.one_row, one = self.constant(1)
        ch = self._vanishing_into((ARITHMETIC_EXT, QUOTIENT_EXT, self.mds_gate, self.swap_gate), zero, one,
                                  lambda t: pi(self.pi_digest + t), lambda t: pi(self.pi_inner + t),
                                  lambda o, t: pi(self.pi_caps + 4 * self.n_cap * o + t), lambda k, l: pi(self.pi_opened + 2 * k + l))
        self.state_cells = list(ch.sponge)
        # the outputs, public: the chain that hashes the public inputs reads them from the cells that hold them
        outs = list(self.zeta_cells) + list(self.gzeta_cells) + self.state_cells
        self.chain_row = self.hash_rows(self.swap_gate, zero, [pi(t) for t in range(self.pi_zeta)] + outs)
        for k, s in enumerate(outs):
            self.public_input(self.pi_zeta + k, s)
        for t in range(4):
            self.tie((self.s_out + t, self.chain_row[-1]), (t, self.pi_row))

    def _vanishing_into(self, gates, zero, one, digest, inner_pi, cap_word, opened):
        """The statement on this builder, with everything it reads given as sources: gates = (the ArithmeticExt gate of n_ops ops, the
        one-op QuotientExt gate, the PoseidonMds gate or None, the PoseidonSwap gate); zero, one: the constants' cells; digest(t): word t
        of the inner circuit digest; inner_pi(t): inner public input t; cap_word(o, t): word t of the flat cap of the wires (0), Z (1)
        and quotient (2) oracle; opened(k, l): limb l of opened value k in the proof's order.  -> the challenger as it leaves, nothing
        pending, zeta drawn last (sipp_amd/plonk_verifier.py's circuit goes on with it).  Sets pih_row, pih_cells, beta_cells,
        gamma_cells, alpha_cells, zeta_cells, gzeta_cells, zeta_n_cells, zh_cells, l0_row, l0_cells, ops, mds_rows, term_cells,
        side_cells, transcript_row."""
        R, D, C, K, W, m, np_ = self.R, self.D, self.C, self.K, self.W, self.m, self.np_
        arithmetic_gate, quotient_gate, mds_gate, swap_gate = gates
        _opened = lambda k: _V(src=(opened(k, 0), opened(k, 1)))
        ZERO, ONE = _V(src=(zero, zero)), _V(src=(one, zero))
        base = lambda s: _V(src=(s, zero))
        # the public-input hash and the transcript
        self.pih_row = self.hash_rows(swap_gate, zero, [inner_pi(t) for t in range(self.n_pi_inner)])
        self.pih_cells = pih = [(self.s_out + t, self.pih_row[-1]) for t in range(4)]
        ch = _Challenger(self, swap_gate, zero, [zero] * 12, [])
        for t in range(4):
            ch.observe(digest(t))
        for s in pih:
            ch.observe(s)
        cap = lambda o: [cap_word(o, t) for t in range(4 * self.n_cap)]
        for s in cap(0):
            ch.observe(s)
        self.beta_cells = [ch.get() for _ in range(C)]
        self.gamma_cells = [ch.get() for _ in range(C)]
        for s in cap(1):
            ch.observe(s)
        self.alpha_cells = [ch.get() for _ in range(C)]
        for s in cap(2):
            ch.observe(s)
        self.zeta_cells = (ch.get(), ch.get())
        self.transcript_row = list(ch.rows)
        beta, gamma, alpha = ([base(s) for s in cells] for cells in (self.beta_cells, self.gamma_cells, self.alpha_cells))
        zeta = _V(src=self.zeta_cells)
        # the opened values
        cv = [_opened(k) for k in range(K)]
        sg = [_opened(K + j) for j in range(R)]
        wv = [_opened(K + R + i) for i in range(W)]
        zs = [_opened(K + R + W + c) for c in range(C)]
        pps = [_opened(K + R + W + C + k) for k in range(C * np_)]
        qs = [_opened(K + R + W + self.nz + k) for k in range(C * D)]
        zs_next = [_opened(self.n0 + c) for c in range(C)]
        ops = self.ops = _Ops(self, arithmetic_gate, self.n_ops, mds_gate)
        mul = lambda a, b: ops.op(1, 0, a, b)
        add = lambda a, b: ops.op(1, 1, a, ONE, b)
        sub = lambda a, b: ops.op(1, -1, a, ONE, b)
        # zeta^n, Z_H, g zeta, L_0
        zeta_n = zeta
        for _ in range(self.inner_log_n):
            zeta_n = mul(zeta_n, zeta_n)
        zh, d1 = sub(zeta_n, ONE), sub(zeta, ONE)
        gzeta = ops.op(_root_of_unity(self.inner_log_n), 0, zeta, ONE)
        ops.flush()
        self.zeta_n_cells, self.zh_cells, self.gzeta_cells = zeta_n.src, zh.src, gzeta.src
        # Z_H = n (zeta - 1) L_0: the generator writes the multiplicand; zeta = 1 writes zero
        self.l0_row = self.new_row(quotient_gate, (1 << self.inner_log_n) % P, 0)
        self.place(self.l0_row, [(0, d1.src[0]), (1, d1.src[1]), (4, zero), (5, zero), (6, zh.src[0]), (7, zh.src[1])])
        l0 = _V(src=((2, self.l0_row), (3, self.l0_row)))
        self.l0_cells = l0.src
        # the terms
        terms = [mul(l0, sub(zs[c], ONE)) for c in range(C)]
        for c in range(C):
            bz = mul(beta[c], zeta)
            wg = [add(wv[j], gamma[c]) for j in range(R)]
            for q in range(m):
                num = zs[c] if q == 0 else pps[c * np_ + q - 1]
                den = zs_next[c] if q == np_ else pps[c * np_ + q]
                for j in range(q * D, min((q + 1) * D, R)):
                    num = mul(num, ops.op(pow(7, j, P), 1, bz, ONE, wg[j]))
                    den = mul(den, ops.op(1, 1, sg[j], beta[c], wg[j]))
                terms.append(sub(num, den))
        terms += self._gate_terms(ops, cv, wv, [base(s) for s in pih], ZERO, ONE)
        # per challenge: Horner in alpha over the terms (last first) against Z_H times Horner in zeta^n over the quotient chunks; with
        # alpha_chunk = K the same sum as Horner inside chunks of K terms, then Horner in alpha^K over the chunk sums
        def horner(ts, x):
            acc = ts[-1]
            for t in ts[-2::-1]:
                acc = ops.op(1, 1, acc, x, t)
            return acc

        def power(x, e):
            """x^e, e >= 2, by squaring from the top bit"""
            acc = x
            for bit in bin(e)[3:]:
                acc = mul(acc, acc)
                if bit == "1":
                    acc = mul(acc, x)
            return acc
        sides = []
        for c in range(C):
            if self.alpha_chunk is None:
                van = horner(terms, alpha[c])
            else:
                sums = [horner(terms[at:at + self.alpha_chunk], alpha[c]) for at in range(0, len(terms), self.alpha_chunk)]
                van = sums[0] if len(sums) == 1 else horner(sums, power(alpha[c], self.alpha_chunk))
            acc = qs[c * D + D - 1]
            for d in range(D - 2, -1, -1):
                acc = ops.op(1, 1, acc, zeta_n, qs[c * D + d])
            sides.append((van, mul(zh, acc)))
        ops.flush()
        self.mds_rows = list(ops.mds_rows)
        self.term_cells = [t.src for t in terms]
        self.side_cells = [(a.src, b.src) for a, b in sides]
        for a, b in self.side_cells:
            for l in range(2):
                self.tie(a[l], b[l])
        return ch

    def _gate_terms(self, ops, cv, wv, pih, ZERO, ONE):
        """the gate compiler -> ngc terms.  Sets gate_monomials (distinct monomials per gate) and gate_ops (ops per gate)"""
        circ, operand = self.inner, {0: wv, 1: cv, 2: pih}
        products, factors, filters = {}, {}, []
        self.gate_monomials, self.gate_ops = [], []

        def product(key):
            if key not in products:
                products[key] = (ONE if not key else operand[key[0][0]][key[0][1]] if len(key) == 1 else
                                 ops.op(1, 0, product(key[:-1]), operand[key[-1][0]][key[-1][1]]))
            return products[key]
        gt = [None] * self.ngc
        for g, (sel, row, lo, hi, _, ncons) in enumerate(circ["gates"]):
            before = ops.made
            f = None
            for i in list(range(lo, hi)) + ([UNUSED] if circ["num_selectors"] > 1 else []):
                if i == row:
                    continue
                if (sel, i) not in factors:
                    factors[sel, i] = ops.op(-1, i, cv[sel], ONE, ONE)             # i - s
                f = factors[sel, i] if f is None else ops.op(1, 0, f, factors[sel, i])
            filters.append(f)
            cons = gate_constraints(circ, g)
            self.gate_monomials.append(len({key for monos in cons for _, key in monos}))
            values = self._poseidon_constraints(ops, wv, ONE) if g in self.routed_gates else None
            for j, monos in enumerate(cons):
                acc = None
                if values is not None:
                    acc = values[j]
                else:
                    for coef, key in monos:
                        acc = ops.op(coef, 0 if acc is None else 1, product(key), ONE, acc)
                if acc is None:
                    continue                                                         # an empty constraint adds nothing
                if f is None:
                    gt[j] = acc if gt[j] is None else ops.op(1, 1, acc, ONE, gt[j])
                else:
                    gt[j] = ops.op(1, 0 if gt[j] is None else 1, f, acc, gt[j])
            self.gate_ops.append(ops.made - before)
        return [ZERO if t is None else t for t in gt]

    def _poseidon_constraints(self, ops, wv, ONE):
        """the 123 constraint values of the Poseidon swap gate at SWAP_LAYOUT, in the program's order, by walking the permutation on the
        opened wires: swap and deltas, the swapped inputs, then the rounds.  Every S-box input but round 0's is an opened wire, so every
        w^7 is there early and a full round's PoseidonMds row reads nothing another row writes; only the 22 partial rounds chain,
        elements 1 .. 11 passing from one row's outputs to the next row's inputs.  The round constants stay off the cells: the state is
        cells + k with k a host-side vector of base-field constants, k <- M k behind an MDS row, and cell + k - wire is made only
        where an element meets a constraint (one op with constants of its own each)"""
        RC, MDS = poseidon_tables()
        lay = SWAP_LAYOUT
        in_, out, sw, delta = [wv[lay["in_"] + i] for i in range(12)], [wv[lay["out"] + i] for i in range(12)], wv[lay["swap"]], lay["delta"]
        mul = lambda a, b: ops.op(1, 0, a, b)
        sub = lambda a, b: ops.op(1, -1, a, ONE, b)

        def pow7(x):
            x2 = mul(x, x)
            return mul(mul(x2, x2), mul(x2, x))
        values = [ops.op(1, -1, sw, sw, sw)]                                       # swap (swap - 1)
        values += [ops.op(1, -1, sw, sub(in_[4 + i], in_[i]), wv[delta + i]) for i in range(4)]
        # round 0 on the swapped inputs (in_i + delta_i, in_(4+i) - delta_i, in_8 .. in_11), its constants added on the cells
        swapped = [ops.op(1, 1, in_[i], ONE, wv[delta + i]) for i in range(4)] + [sub(in_[4 + i], wv[delta + i]) for i in range(4)] + in_[8:]
        state = ops.mds([pow7(ops.op(RC[i], 1, ONE, ONE, swapped[i])) for i in range(12)])
        k = [0] * 12
        met = lambda cell, kk, wire: ops.op(kk, 1, ONE, ONE, sub(cell, wire))      # cell + k - wire
        for rnd in range(1, 30):
            k = [(k[i] + RC[12 * rnd + i]) % P for i in range(12)]
            for i in (range(12) if rnd < 4 or rnd >= 26 else (0,)):
                w = wv[sbox_wire(lay["sbox"], rnd, i)]
                values.append(met(state[i], k[i], w))
                state[i], k[i] = pow7(w), 0
            state = ops.mds(state)
            k = [sum(MDS[r][c] * k[c] for c in range(12)) % P for r in range(12)]
        values += [met(state[i], k[i], out[i]) for i in range(12)]
        assert len(values) == 123
        return values

    # ---- the values ----
    def _check(self, digest, inner_pis, caps, opened):
        digest, inner_pis = [int(v) % P for v in digest], [int(v) % P for v in inner_pis]
        caps = [np.asarray(c, dtype=np.uint64).reshape(self.n_cap, 4) for c in caps]
        opened = [(int(v[0]) % P, int(v[1]) % P) for v in opened]
        assert len(digest) == 4 and len(inner_pis) == self.n_pi_inner and len(caps) == 3 and len(opened) == self.n_open
        return digest, inner_pis, caps, opened

    def transcript(self, digest, inner_pis, caps):
        """what the circuit's challenger draws and leaves, by the library's host permutation -> dict(pih, betas, gammas, alphas, zeta,
        gzeta, state)"""
        ch = _HostChallenger()
        pih = ch.hash_no_pad(inner_pis)
        for v in list(digest) + pih + [int(x) for x in np.asarray(caps[0]).reshape(-1)]:
            ch.observe(v)
        betas = [ch.get() for _ in range(self.C)]
        gammas = [ch.get() for _ in range(self.C)]
        for v in np.asarray(caps[1]).reshape(-1):
            ch.observe(int(v))
        alphas = [ch.get() for _ in range(self.C)]
        for v in np.asarray(caps[2]).reshape(-1):
            ch.observe(int(v))
        zeta = (ch.get(), ch.get())
        g = _root_of_unity(self.inner_log_n)
        return {"pih": pih, "betas": betas, "gammas": gammas, "alphas": alphas, "zeta": zeta, "gzeta": (zeta[0] * g % P, zeta[1] * g % P),
                "state": list(ch.state)}

    def public_inputs(self, digest, inner_pis, caps, opened):
        """digest || inner public inputs || the three caps || the opened values || zeta || g zeta || the departing state, as ints"""
        digest, inner_pis, caps, opened = self._check(digest, inner_pis, caps, opened)
        t = self.transcript(digest, inner_pis, caps)
        out = digest + inner_pis + [int(v) for c in caps for v in c.reshape(-1)] + [l for v in opened for l in v]
        out += list(t["zeta"]) + list(t["gzeta"]) + t["state"]
        assert len(out) == self.n_pi
        return out

    def input_cells(self, digest, inner_pis, caps, opened):
        """(cells, values): every cell on the cycle of a public input in front of zeta, once; the outputs are generated"""
        pis = self.public_inputs(digest, inner_pis, caps, opened)
        cycles = self.pi_cycle[:self.pi_zeta]
        return (np.array([x for cyc in cycles for x in cyc], dtype=np.uint64),
                np.array([pis[t] for t, cyc in enumerate(cycles) for _ in cyc], dtype=np.uint64))

    def partial_witness(self, digest, inner_pis, caps, opened):
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        cells, vals = self.input_cells(digest, inner_pis, caps, opened)
        w.reshape(-1)[cells.astype(np.int64)] = vals
        return w

    # ---- the flat proof ----
    def proof_layout(self, proof_words):
        """a flat "SIPPPLK3" proof of proof_words words -> (cells, word index, pi_word): every input cell once with the offset of its
        value in proof || digest, and per public input the offset of its value there, -1 for the outputs"""
        opened_at = HEADER_WORDS + 3 * 4 * self.n_cap + FRI_HEADER_WORDS
        pi_word = np.full(self.n_pi, -1, dtype=np.int64)
        pi_word[self.pi_digest:self.pi_digest + 4] = proof_words + np.arange(4)
        pi_word[self.pi_inner:self.pi_inner + self.n_pi_inner] = proof_words - self.n_pi_inner + np.arange(self.n_pi_inner)
        pi_word[self.pi_caps:self.pi_opened] = HEADER_WORDS + np.arange(3 * 4 * self.n_cap)
        pi_word[self.pi_opened:self.pi_zeta] = opened_at + np.arange(2 * self.n_open)
        cycles = self.pi_cycle[:self.pi_zeta]
        return (np.array([x for cyc in cycles for x in cyc], dtype=np.uint64),
                np.array([pi_word[t] for t, cyc in enumerate(cycles) for _ in cyc], dtype=np.uint64), pi_word)


def flat_proof_arguments(circ, proof, digest):
    """the argument tuple of PlonkVanishingCircuit.public_inputs / partial_witness / input_cells from a flat inner proof"""
    pf = [int(v) for v in proof]
    n_cap, at = circ.n_cap, HEADER_WORDS
    caps = [np.array(pf[at + 4 * n_cap * o:at + 4 * n_cap * (o + 1)], dtype=np.uint64).reshape(n_cap, 4) for o in range(3)]
    at += 3 * 4 * n_cap + FRI_HEADER_WORDS
    opened = [(pf[at + 2 * k], pf[at + 2 * k + 1]) for k in range(circ.n_open)]
    return (list(digest), pf[len(pf) - circ.n_pi_inner:], caps, opened)


class PlonkVanishingProver(CircuitProver):
    """PlonkVanishingCircuit through the library's CircuitData: prove(*arguments), or prove_proof(flat inner proof, digest), which
    sends the proof's words and lets the device gather the input cells (sipp_circuit_prove_words)"""

    def __init__(self, ctx, *shape, fri=None, params=None, digest=None, **kw):
        super().__init__(ctx, PlonkVanishingCircuit(*shape, **kw), fri, params, digest)
        self._layout = None

    def prove(self, *inputs):
        c = self.circ
        cells, values = c.input_cells(*inputs)
        return self.data.prove_inputs(cells, values, c.public_inputs(*inputs))

    def prove_proof(self, proof, digest):
        from ._lib import refuse_keccak_proof
        refuse_keccak_proof(proof, "PlonkVanishingProver")
        c = self.circ
        proof = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1)
        if self._layout is None or self._layout[0] != len(proof):
            cells, words, pi_word = c.proof_layout(len(proof))
            self.data.set_input_map(cells, words, len(proof), 4)
            self._layout = (len(proof), pi_word)
        extra = np.array([int(v) % P for v in digest], dtype=np.uint64)
        staged, pi_word = np.concatenate([proof, extra]), self._layout[1]
        pis = np.empty(c.n_pi, dtype=np.uint64)
        pis[:c.pi_zeta] = staged[pi_word[:c.pi_zeta]]
        n_cap = c.n_cap
        caps = [proof[HEADER_WORDS + 4 * n_cap * o:HEADER_WORDS + 4 * n_cap * (o + 1)] for o in range(3)]
        t = c.transcript(extra, proof[len(proof) - c.n_pi_inner:], caps)
        pis[c.pi_zeta:] = np.array(list(t["zeta"]) + list(t["gzeta"]) + t["state"], dtype=np.uint64)
        return self.data.prove_words(proof, extra, pis)


class PlonkProofVerifier:
    """Both halves of plonky2's verify for one inner circuit, as two outer circuits: the vanishing circuit above and a FriProofCircuit
    (sipp_amd/fri_proof.py) over the inner proof's opening section -- oracles of K + R, W, C (1 + np) and C D columns, batch 0 every
    column at zeta, batch 1 the C columns of Z at g zeta, nothing pending in the arriving transcript.  The pair is accepted only if both
    proofs verify and their shared public inputs agree word for word (verify); joining the two into one circuit is not done here.

    inner_fri: the inner proofs' FRI parameters (sipp_amd.FriParams: one arity for every round).  ctx carries the vanishing circuit's
    data, fri_ctx (default: ctx) the FRI circuit's; fri (None, or one FriParams per outer circuit: they differ in size), outer_params
    and digest are the OUTER proofs'."""

    def __init__(self, ctx, log_n, params, circuit, inner_fri, n_pi_inner, fri_ctx=None, fri=None, outer_params=None, digest=None, min_log_n=10,
                 verifier_data=None, poseidon_mds=False, alpha_chunk=None):
        """poseidon_mds, alpha_chunk: the vanishing circuit's; they are part of the verifier's shape (another setting is another circuit,
        with another constants_sigmas cap).
        ctx = None builds the verifying half alone (no device): verifier_data = per outer circuit its (constants_sigmas cap, digest),
        fri and outer_params as the provers had them"""
        from . import _lib
        from .fri_proof import FriProofCircuit, FriProofProver
        cap_height = min(inner_fri.cap_height, log_n + inner_fri.rate_bits)
        R, D, C = ((params.num_routed_wires, params.max_degree, params.num_challenges) if hasattr(params, "max_degree") else
                   tuple(int(x) for x in params))
        K, W, m = circuit["num_constants"], circuit["num_wires"], -(-R // D)
        n0, z0 = K + R + W + C * m + C * D, K + R + W
        arity = [int(inner_fri.arity_bits[r]) for r in range(inner_fri.n_rounds)]
        v_shape = (log_n, (R, D, C), circuit, cap_height, n_pi_inner)
        v_kw = dict(min_log_n=min_log_n, poseidon_mds=poseidon_mds, alpha_chunk=alpha_chunk)
        f_shape = (log_n + inner_fri.rate_bits, cap_height, [K + R, W, C * m, C * D], [list(range(n0)), list(range(z0, z0 + C))], arity,
                   inner_fri.n_rounds, (1 << log_n) >> sum(arity), inner_fri.num_queries)
        f_kw = dict(min_log_n=min_log_n, pow_bits=inner_fri.pow_bits, pow_rule=inner_fri.pow_rule, n_in=0)
        self.vanishing = self.fri = None
        fri = (None, None) if fri is None else tuple(fri)
        if ctx is None:
            assert verifier_data is not None and None not in fri
            self.vc, self.fc = PlonkVanishingCircuit(*v_shape, **v_kw), FriProofCircuit(*f_shape, **f_kw)
            self.verifier_data = [(np.asarray(cap, dtype=np.uint64).reshape(-1), np.array([int(x) for x in dg], dtype=np.uint64))
                                  for cap, dg in verifier_data]
            self.outer_fri = fri
        else:
            self.vanishing = PlonkVanishingProver(ctx, *v_shape, fri=fri[0], params=outer_params, digest=digest, **v_kw)
            try:
                self.fri = FriProofProver(fri_ctx or ctx, *f_shape, fri=fri[1], params=outer_params, digest=digest, **f_kw)
            except Exception:
                self.vanishing.close()
                raise
            self.vc, self.fc = self.vanishing.circ, self.fri.circ
            self.verifier_data = [(pr.cap.reshape(-1), pr.digest) for pr in (self.vanishing, self.fri)]
            self.outer_fri = (self.vanishing.fri, self.fri.fri)
        self.outer_params = outer_params if outer_params is not None else _lib.PlonkParams(self.vc.num_routed, 8, 2)
        self._pc = [_lib.PlonkCircuit.from_dict(c.circuit()) for c in (self.vc, self.fc)]

    def _verdict(self, which, proof):
        """sipp_plonk_verify_gates (host code) with outer circuit `which`'s verifier data -> (status, refusing stage)"""
        import ctypes as C
        from . import _lib
        pf = np.ascontiguousarray(proof, dtype=np.uint64)
        cap, dg = self.verifier_data[which]
        reason = C.c_int(0)
        u64p = C.POINTER(C.c_uint64)
        rc = _lib.lib().sipp_plonk_verify_gates(pf.ctypes.data_as(u64p), len(pf), cap.ctypes.data_as(u64p), C.byref(self.outer_params),
                                                C.byref(self.outer_fri[which]), C.byref(self._pc[which]), dg.ctypes.data_as(u64p), C.byref(reason))
        return rc, reason.value

    def section(self, proof):
        """the opening section of a flat inner proof: what lies between the caps and the public inputs"""
        at = HEADER_WORDS + 3 * 4 * self.vc.n_cap
        return proof[at:len(proof) - self.vc.n_pi_inner]

    def prove_proof(self, inner_proof, constants_sigmas_cap, digest):
        """-> (the vanishing circuit's proof, the FRI circuit's proof)"""
        from ._lib import refuse_keccak_proof
        refuse_keccak_proof(inner_proof, "PlonkProofVerifier")
        v = self.vc
        proof = np.ascontiguousarray(inner_proof, dtype=np.uint64).reshape(-1)
        first = self.vanishing.prove_proof(proof, digest)
        pis = first[len(first) - v.n_pi:]
        at = HEADER_WORDS
        caps = [np.asarray(constants_sigmas_cap, dtype=np.uint64).reshape(-1)] + [proof[at + 4 * v.n_cap * o:at + 4 * v.n_cap * (o + 1)] for o in range(3)]
        points = [pis[v.pi_zeta:v.pi_zeta + 2], pis[v.pi_gzeta:v.pi_gzeta + 2]]
        second = self.fri.prove_proof(self.section(proof), caps, points, (pis[v.pi_state:v.pi_state + 12], []))
        return first, second

    def shared(self, pair):
        """the public inputs both proofs carry, side by side: [(what, the vanishing proof's words, the FRI proof's words)]"""
        v, f = self.vc, self.fc
        a, b = ([int(x) for x in pf[len(pf) - c.n_pi:]] for pf, c in zip(pair, (v, f)))
        opened = a[v.pi_opened:v.pi_zeta]
        fb = lambda k, lo, n: b[f.pi_batch[k] + lo:f.pi_batch[k] + lo + n]
        return [("state", a[v.pi_state:v.pi_state + 12], b[:12]),
                ("zeta", a[v.pi_zeta:v.pi_zeta + 2], fb(0, 0, 2)), ("gzeta", a[v.pi_gzeta:v.pi_gzeta + 2], fb(1, 0, 2)),
                ("opened", opened[:2 * v.n0], fb(0, 2, 2 * v.n0)), ("opened_next", opened[2 * v.n0:], fb(1, 2, 2 * v.C)),
                ("caps", a[v.pi_caps:v.pi_opened], b[f.pi_caps + 4 * v.n_cap:f.pi_caps + 4 * 4 * v.n_cap])]

    def verify(self, pair, constants_sigmas_cap, digest):
        """-> the inner public inputs; raises ValueError naming what refuses the pair"""
        v, f = self.vc, self.fc
        for which, (name, c, pf) in enumerate((("vanishing", v, pair[0]), ("fri", f, pair[1]))):
            if len(pf) < c.n_pi:
                raise ValueError("the %s proof is too short" % name)
            verdict = self._verdict(which, pf)
            if verdict != (0, 0):
                raise ValueError("the %s proof is refused: status %d at stage %d" % ((name,) + tuple(verdict)))
        for what, x, y in self.shared(pair):
            if x != y:
                raise ValueError("the two proofs differ in their %s" % what)
        a, b = ([int(x) for x in pf[len(pf) - c.n_pi:]] for pf, c in zip(pair, (v, f)))
        if b[f.pi_caps:f.pi_caps + 4 * v.n_cap] != [int(x) for x in np.asarray(constants_sigmas_cap, dtype=np.uint64).reshape(-1)]:
            raise ValueError("the FRI proof opens another constants_sigmas cap")
        if a[v.pi_digest:v.pi_digest + 4] != [int(x) % P for x in digest]:
            raise ValueError("the vanishing proof is for another circuit digest")
        return a[v.pi_inner:v.pi_inner + v.n_pi_inner]

    def close(self):
        for pr in (self.vanishing, self.fri):
            if pr is not None:
                pr.close()
