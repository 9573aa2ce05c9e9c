"""Merkle openings in the outer circuit: plonky2's PoseidonGate WITH its swap wire as a gate program, and a circuit that proves openings of
a commitment against its cap (what the recursive verifier does for every FRI query: hash the opened leaf, walk the sibling path).

  poseidon_swap_gate()      the 123 constraints of upstream's PoseidonGate (gates/poseidon.rs, recalled) in the program words of
                            sipp_plonk_circuit (include/sipp_hip.h, "gates as data"), upstream's order and sign
  declare_swap_gate()       that gate in a circuit's gate set, in SWAP_LAYOUT (every circuit hashes its public inputs with it)
  poseidon_mds_gate()       upstream's PoseidonMdsGate (gates/poseidon_mds.rs, recalled): the linear layer on twelve extension elements, 24
                            constraints of degree 1; declare_mds_gate() puts it into a gate set (sipp_amd/plonk_vanishing.py's route)
  opening_into()            the wiring of one opening on any builder, its leaf, index bits and cap given as sources: this circuit's
                            paths and those of sipp_amd/fri_verifier.py
  MerkleOpeningCircuit      the statement "for each path k, leaves[k] sits at index idx[k] of the tree whose cap is `cap`" as calls of
                            sipp_amd/circuit.py's CircuitBuilder, which makes the rows, the copy cycles (sigmas), the generators and
                            the level schedule of it
  MerkleOpeningProver       the circuit through the library's CircuitData: built once, then prove(cap, idx, leaves, siblings) / verify

Statement layout.  Public inputs = cap (2^cap_height digests, flat) || per path (idx >> height, idx mod 2^height, leaf values).  They
are hashed IN CIRCUIT by a chain of swap-0 Poseidon rows (hash_n_to_hash_no_pad, overwrite mode) whose final digest is copy-constrained
to the PublicInput gate's four wires, which the prover binds to hash_no_pad(public inputs): the cap, the indices and the leaves are
therefore the verifier's, not free witness.  Per path: a BaseSum row with 1-bit limbs splits the low index into its bits; the leaf hash
(hash_or_noop) is a chain of swap-0 rows; `height` swap rows walk the path (digest in 0 .. 3 by copy, sibling in 4 .. 7, capacity 0,
swap = bit l); RandomAccess copies select cap[idx >> height] word by word, and their claimed words are the root's by copy constraint.

numpy only; imports nothing from the test oracle."""
import os

import numpy as np

from .circuit import SWAP_LAYOUT, fri_params  # noqa: F401 (used from here by tests and scripts)
from .circuit import (BASE_SUM, GEN_POSEIDON_MDS, GEN_POSEIDON_SWAP, GEN_RANDOM_ACCESS, P, PUBLIC_INPUT, CircuitBuilder, CircuitProver, _Prog,
                      _W, pi, random_access_into)

GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "RandomAccess", "PoseidonSwap"]
GATE_GROUP = (0, 0, 0, 0, 1, 2)                 # RandomAccess (degree cap_height + 1) and PoseidonSwap (degree 7) alone in their groups
RANDOM_ACCESS, POSEIDON_SWAP = 4, 5
_TABLES = None


def poseidon_tables():
    """(ALL_ROUND_CONSTANTS[360], MDS rows): data/poseidon_goldilocks_rc.txt and the circulant-plus-diagonal matrix"""
    global _TABLES
    if _TABLES is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        vals = []
        for line in open(os.path.join(root, "data", "poseidon_goldilocks_rc.txt")):
            vals += [int(t, 16) for t in line.split("#")[0].replace(",", " ").split()]
        assert len(vals) == 360
        circ = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
        rows = [tuple(circ[(c - r) % 12] + (8 if r == c == 0 else 0) for c in range(12)) for r in range(12)]
        _TABLES = (vals, rows)
    return _TABLES


def sbox_wire(sbox, rnd, i):
    """the wire holding the S-box INPUT of state element i in round rnd (1 .. 29), relative layout of SIPP_GEN_POSEIDON[_SWAP]"""
    if 1 <= rnd <= 3:
        return sbox + 12 * (rnd - 1) + i
    if 4 <= rnd <= 25:
        assert i == 0
        return sbox + 36 + (rnd - 4)
    assert 26 <= rnd <= 29
    return sbox + 58 + 12 * (rnd - 26) + i


def _multinomial(a, b, e):
    from math import factorial
    return factorial(a + b + e) // (factorial(a) * factorial(b) * factorial(e))


def swap_gate_into(pr, in_, out, swap, delta, sbox):
    RC, MDS = poseidon_tables()
    sw = (_W, swap)
    pr.constraint([(1, [sw, sw]), (-1, [sw])])                                        # swap (swap - 1)
    for i in range(4):                                                                # swap (in[4+i] - in[i]) - delta_i
        pr.constraint([(1, [sw, (_W, in_ + 4 + i)]), (-1, [sw, (_W, in_ + i)]), (-1, [(_W, delta + i)])])

    def mds(st):
        res = []
        for r in range(12):
            f = {}
            for c in range(12):
                for atom, v in st[c].items():
                    f[atom] = (f.get(atom, 0) + MDS[r][c] * v) % P
            res.append(f)
        return res
    # symbolic state: linear forms over the atoms ('b', i) = (swapped in_i + rc_0,i)^7, ('w', k) = wire_k^7, 'one'
    state = mds([{("b", i): 1} for i in range(12)])
    cons = []
    for rnd in range(1, 30):
        full = rnd < 4 or rnd >= 26
        for i in range(12):
            state[i] = dict(state[i])
            state[i]["one"] = (state[i].get("one", 0) + RC[12 * rnd + i]) % P
        for i in (range(12) if full else (0,)):
            w = sbox_wire(sbox, rnd, i)
            cons.append((state[i], w))
            state[i] = {("w", w): 1}
        state = mds(state)
    for i in range(12):
        cons.append((state[i], out + i))
    for form, target in cons:                                                         # state_form - wire
        monos = [(form.get("one", 0), [])]
        for atom, coef in form.items():
            if atom == "one":
                continue
            if atom[0] == "w":
                monos.append((coef, [(_W, atom[1])] * 7))
                continue
            # (u + sgn v + c)^7 over the swapped input: u = in_i, v = delta_(i mod 4), sgn = +1 (i < 4) / -1 (4 <= i < 8); no v for i >= 8
            i, c = atom[1], RC[atom[1]]
            u = (_W, in_ + i)
            v, sgn = ((_W, delta + i), 1) if i < 4 else ((_W, delta + i - 4), -1) if i < 8 else (None, 0)
            for a in range(8):
                for b in range(8 - a if v else 1):
                    e = 7 - a - b
                    m = coef * _multinomial(a, b, e) * pow(c, e, P) * (sgn ** b if b else 1)
                    monos.append((m, [u] * a + [v] * b))
        monos.append((-1, [(_W, target)]))
        pr.constraint(monos)


def poseidon_swap_gate(in_=0, out=12, swap=24, delta=25, sbox=29):
    """upstream PoseidonGate's constraints as program words (np.int64): swap (swap - 1); swap (in[4+i] - in[i]) - delta_i, i < 4; the S-box
    inputs of rounds 1 .. 3 (36), 4 .. 25 (22, element 0), 26 .. 29 (48); the 12 outputs -- 123, each  state_form - wire.  Round 0 works on
    the swapped inputs: its atoms (in_i +- delta_i + rc)^7 expand in two wires."""
    pr = _Prog()
    swap_gate_into(pr, in_, out, swap, delta, sbox)
    assert pr.count == 123
    return np.array(pr.words, dtype=np.int64)


def declare_swap_gate(b, index):
    """the swap gate as gate `index` of builder b, in SWAP_LAYOUT"""
    b.declare(index, 7, (GEN_POSEIDON_SWAP, b.s_in, b.s_out, b.s_sbox, b.s_swap, b.s_delta), swap_gate_into, b.s_in, b.s_out, b.s_swap,
              b.s_delta, b.s_sbox)


def mds_gate_into(pr, in_, out):
    _, MDS = poseidon_tables()
    for r in range(12):
        for l in range(2):
            pr.constraint([(MDS[r][c], [(_W, in_ + 2 * c + l)]) for c in range(12)] + [(-1, [(_W, out + 2 * r + l)])])


def poseidon_mds_gate(in_=0, out=24):
    """upstream PoseidonMdsGate's constraints as program words (np.int64): twelve extension elements, element c limb l at in_ + 2 c + l,
    and their image under the permutation's MDS matrix at out + 2 r + l -- 24 constraints of degree 1, constraint 2 r + l =
    sum_c M[r][c] in[2 c + l] - out[2 r + l]  (the matrix is over the base field: the limbs do not mix)"""
    pr = _Prog()
    mds_gate_into(pr, in_, out)
    assert pr.count == 24
    return np.array(pr.words, dtype=np.int64)


def declare_mds_gate(b, index, in_=0, out=24):
    """the MDS gate as gate `index` of builder b (SIPP_GEN_POSEIDON_MDS): all 48 cells are routed"""
    assert in_ + 24 <= b.num_routed and out + 24 <= b.num_routed and (in_ + 24 <= out or out + 24 <= in_)
    b.declare(index, 1, (GEN_POSEIDON_MDS, in_, out), mds_gate_into, in_, out)


def opening_into(b, ra_shape, swap_gate, zero, leaf, swap_bits, index, cap_word, cap_bits=None, sibling=None):
    """One Merkle opening on builder b: the leaf (sources) sits under the cap at the index whose low bits are the cells swap_bits, one per
    level of the path (none: the tree is its cap), and whose high part is the source `index`.  ra_shape = (gate, rows, copies per row,
    stride, cap entries) of the cap selection; cap_word(j, q) = the source of word q of cap entry j.  cap_bits: the cells the selection's
    bit wires are tied to (the high bits of a split the caller made; None: the generator's bits stand alone, `index` is bound elsewhere).
    sibling(l, t): the source of word t of the sibling at level l (None: the cells stay free input cells).
    -> (the RandomAccess rows, the leaf-hash rows, the path rows)"""
    s_in, s_out = b.s_in, b.s_out
    ra_gate, ra_rows, ra_copies, ra_stride, n_cap = ra_shape
    ra = [b.new_row(ra_gate) for _ in range(ra_rows)]
    # the leaf hash (hash_or_noop): at most 4 values are their own digest, padded with zero
    rows = b.hash_rows(swap_gate, zero, leaf) if len(leaf) > 4 else []
    digest = [(s_out + t, rows[-1]) if rows else leaf[t] if t < len(leaf) else zero for t in range(4)]
    # the path: digest in 0 .. 3, the sibling (an input) in 4 .. 7, capacity 0, swap = bit l of the low index
    path = []
    for l, bit in enumerate(swap_bits):
        r = b.new_row(swap_gate)
        sib = [(s_in + 4 + t, sibling(l, t)) for t in range(4)] if sibling else []
        b.place(r, [(s_in + t, digest[t]) for t in range(4)] + sib + [(s_in + t, zero) for t in range(8, 12)] + [(b.s_swap, bit)])
        digest = [(s_out + t, r) for t in range(4)]
        path.append(r)
    # cap selection: copy q selects digest word q of the cap entry; the root word is the claimed word (both generated: no copy)
    for i, r in enumerate(ra):
        feeds = []
        for cp in range(ra_copies):
            at, q = ra_stride * cp, ra_copies * i + cp
            feeds += [(at, index)] + [(at + 2 + j, cap_word(j, q)) for j in range(n_cap)]
            b.tie(digest[q], (at + 1, r))
            for l, bit in enumerate(cap_bits or ()):
                b.tie(bit, (at + 2 + n_cap + l, r))
        b.place(r, feeds)
    return ra, rows, path


class MerkleOpeningCircuit(CircuitBuilder):
    """The circuit of n_paths openings of leaves of leaf_len values, paths of `height` siblings, under a cap of 2^cap_height digests.
    Cells are wire * N + row; every cell that copy constraints tie together lies on one permutation cycle."""
    n_public_args = 3                                           # public_inputs takes partial_witness's arguments without the siblings

    def __init__(self, leaf_len, height, cap_height, n_paths, num_wires=135, num_routed=80, min_log_n=10):
        assert leaf_len >= 1 and n_paths >= 1 and 1 <= height and 1 + height <= num_routed and height <= 32
        assert 1 <= cap_height <= 6 and num_wires >= 135 and num_routed >= 29
        self.leaf_len, self.height, self.cap_height, self.n_paths = leaf_len, height, cap_height, n_paths
        self.n_cap = 1 << cap_height
        super().__init__(num_wires, num_routed, GATE_NAMES, GATE_GROUP, 1, 4 * self.n_cap + n_paths * (2 + leaf_len))
        # RandomAccess: per copy index, claimed, 2^cap_height items, cap_height bits (interleaved, SIPP_GEN_RANDOM_ACCESS); the routed cells of
        # every copy stay below num_routed; copies per row divide 4 (one digest word per copy)
        self.ra_stride = 2 + self.n_cap + cap_height
        self.ra_copies = next(c for c in (4, 2, 1) if (c - 1) * self.ra_stride + 2 + self.n_cap <= num_routed)
        self.ra_rows = 4 // self.ra_copies
        self.n_leaf_rows = 0 if leaf_len <= 4 else -(-leaf_len // 8)
        self.declare_basic(height)
        self.declare(RANDOM_ACCESS, cap_height + 1, (GEN_RANDOM_ACCESS, self.ra_copies, self.ra_stride, cap_height), random_access_into,
                     self.ra_copies, self.ra_stride, cap_height)
        declare_swap_gate(self, POSEIDON_SWAP)
        self._wiring()
        self.finish(min_log_n)
        # the input cells the partial witness sets besides the public inputs' cycles: the siblings
        self.sibling_cells = [[[(self.s_in + 4 + t) * self.n + r for t in range(4)] for r in rows] for rows in self.path_row]

    def _wiring(self):
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.const_row, zero = self.constant(0)
        self.bs_row, self.ra_row, self.leaf_row, self.path_row = [], [], [], []
        ra_shape = (RANDOM_ACCESS, self.ra_rows, self.ra_copies, self.ra_stride, self.n_cap)
        for k in range(self.n_paths):
            hi_t = 4 * self.n_cap + k * (2 + self.leaf_len)
            lo_t, leaf_t = hi_t + 1, hi_t + 2
            # the index bits
            bs = self.new_row(BASE_SUM)
            self.place(bs, [(0, pi(lo_t))])
            ra, leaf, path = opening_into(self, ra_shape, POSEIDON_SWAP, zero, [pi(leaf_t + t) for t in range(self.leaf_len)],
                                          [(1 + l, bs) for l in range(self.height)], pi(hi_t), lambda j, q: pi(4 * j + q))
            self.bs_row.append(bs); self.ra_row.append(ra); self.leaf_row.append(leaf); self.path_row.append(path)
        self.hash_public_inputs(POSEIDON_SWAP, zero)

    def _check(self, cap, idx, leaves, siblings=None):
        cap = np.asarray(cap, dtype=np.uint64).reshape(self.n_cap, 4)
        idx = [int(x) for x in idx]
        assert len(idx) == self.n_paths and all(0 <= x < (self.n_cap << self.height) for x in idx)
        leaves = np.asarray(leaves, dtype=np.uint64).reshape(self.n_paths, self.leaf_len)
        if siblings is not None:
            siblings = np.asarray(siblings, dtype=np.uint64).reshape(self.n_paths, self.height, 4)
        return cap, idx, leaves, siblings

    def public_inputs(self, cap, idx, leaves):
        """cap || per path (idx >> height, idx mod 2^height, leaf values), as ints"""
        cap, idx, leaves, _ = self._check(cap, idx, leaves)
        out = [int(x) for x in cap.reshape(-1)]
        for k in range(self.n_paths):
            out += [idx[k] >> self.height, idx[k] & ((1 << self.height) - 1)] + [int(x) for x in leaves[k]]
        return out

    def partial_witness(self, cap, idx, leaves, siblings):
        """[num_wires][N] with the INPUT cells set (plonky2's PartialWitness): every cell on a cycle of a public input, the siblings;
        everything else 0 (the generators and the schedule's copies fill it)"""
        cap, idx, leaves, siblings = self._check(cap, idx, leaves, siblings)
        w, flat = self.public_input_witness(self.public_inputs(cap, idx, leaves))
        for k in range(self.n_paths):
            for l in range(self.height):
                flat[np.asarray(self.sibling_cells[k][l], dtype=np.int64)] = siblings[k, l]
        return w


class MerkleOpeningProver(CircuitProver):
    """MerkleOpeningCircuit through the library's CircuitData: built once, then prove(cap, idx, leaves, siblings) / verify"""

    def __init__(self, ctx, leaf_len, height, cap_height, n_paths, fri=None, params=None, digest=None, min_log_n=10):
        super().__init__(ctx, MerkleOpeningCircuit(leaf_len, height, cap_height, n_paths, min_log_n=min_log_n), fri, params, digest)
