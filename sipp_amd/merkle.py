"""Merkle openings in the outer circuit: plonky2's PoseidonGate WITH its swap wire as a gate program, and a circuit that proves openings of
a commitment against its cap (what the recursive verifier does for every FRI query: hash the opened leaf, walk the sibling path).

  poseidon_swap_gate()      the 123 constraints of upstream's PoseidonGate (gates/poseidon.rs, recalled) in the program words of
                            sipp_plonk_circuit (include/sipp_hip.h, "gates as data"), upstream's order and sign
  MerkleOpeningCircuit      the gate set, the rows, the copy cycles (sigmas), the generators and the level schedule of the statement
                            "for each path k, leaves[k] sits at index idx[k] of the tree whose cap is `cap`"
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

P = 0xFFFFFFFF00000001
PP = np.uint64(P)
M32 = np.uint64(0xFFFFFFFF)
EPS = np.uint64(0xFFFFFFFF)
UNUSED = 0xFFFFFFFF

# include/sipp_hip.h SIPP_GEN_*
GEN_BASE_SPLIT, GEN_CONSTANT, GEN_PUBLIC_INPUT, GEN_RANDOM_ACCESS, GEN_POSEIDON_SWAP = 2, 3, 4, 6, 9
# program factor kinds
_W, _K, _PIH = 0, 1, 2
# upstream's PoseidonGate layout: 135 wires
SWAP_LAYOUT = {"in_": 0, "out": 12, "swap": 24, "delta": 25, "sbox": 29}
GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "RandomAccess", "PoseidonSwap"]
NOOP, PUBLIC_INPUT, CONSTANT, BASE_SUM, RANDOM_ACCESS, POSEIDON_SWAP = range(6)
_C0 = 3                                         # the constant column behind the three selector columns (the Constant gate's value)


# ---- Goldilocks over numpy (sigmas only) ----------------------------------------------------------------------------------------------
def _gl_mul(a, b):
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    a0, a1, b0, b1 = a & M32, a >> np.uint64(32), b & M32, b >> np.uint64(32)
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = lh + hl
    cmid = (mid < lh).astype(np.uint64)
    lo = ll + (mid << np.uint64(32))
    clo = (lo < ll).astype(np.uint64)
    hi = hh + (mid >> np.uint64(32)) + (cmid << np.uint64(32)) + clo
    h0, h1 = hi & M32, hi >> np.uint64(32)
    t0 = lo - h1
    t0 = np.where(lo < h1, t0 - EPS, t0)
    t1 = (h0 << np.uint64(32)) - h0
    r = t0 + t1
    r = np.where(r < t1, r + EPS, r)
    return np.where(r >= PP, r - PP, r)


def _powers(base, n):
    out = np.ones(n, dtype=np.uint64)
    m, b = 1, int(base)
    while m < n:
        out[m:2 * m] = _gl_mul(out[:m], np.uint64(b))
        b = b * b % P
        m *= 2
    return out


def _root_of_unity(log_n):
    return pow(1753635133440165772, 1 << (32 - log_n), P)


def _i64(c):
    c %= P
    return c if c < (1 << 63) else c - P


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


class _Prog:
    """program words of sipp_plonk_circuit: per constraint n_mono, then per monomial coef, n_factors, (kind, index) x n_factors"""

    def __init__(self):
        self.words = []
        self.count = 0

    def constraint(self, monos):
        merged = {}
        for coef, factors in monos:
            key = tuple(sorted(factors))
            merged[key] = (merged.get(key, 0) + coef) % P
        items = [(c, k) for k, c in merged.items() if c]
        self.words.append(len(items))
        for coef, factors in items:
            self.words.extend([_i64(coef), len(factors)])
            for kind, idx in factors:
                self.words.extend([kind, idx])
        self.count += 1


def _multinomial(a, b, e):
    from math import factorial
    return factorial(a + b + e) // (factorial(a) * factorial(b) * factorial(e))


def _swap_gate_into(pr, in_, out, swap, delta, sbox):
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
    _swap_gate_into(pr, in_, out, swap, delta, sbox)
    assert pr.count == 123
    return np.array(pr.words, dtype=np.int64)


class MerkleOpeningCircuit:
    """The circuit of n_paths openings of leaves of leaf_len values, paths of `height` siblings, under a cap of 2^cap_height digests.
    Cells are wire * N + row; every cell that copy constraints tie together lies on one permutation cycle."""

    def __init__(self, leaf_len, height, cap_height, n_paths, num_wires=135, num_routed=80, min_log_n=10):
        # min_log_n: the device prover's FRI takes degree bits 10 .. 24; smaller circuits are padded with Noop rows
        assert leaf_len >= 1 and n_paths >= 1 and 1 <= height and 1 + height <= num_routed and height <= 32
        assert 1 <= cap_height <= 6 and num_wires >= 135 and num_routed >= 29
        self.leaf_len, self.height, self.cap_height, self.n_paths = leaf_len, height, cap_height, n_paths
        self.num_wires, self.num_routed = num_wires, num_routed
        lay = SWAP_LAYOUT
        self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox = lay["in_"], lay["out"], lay["swap"], lay["delta"], lay["sbox"]
        # RandomAccess: per copy index, claimed, 2^cap_height items, cap_height bits (interleaved, SIPP_GEN_RANDOM_ACCESS); the routed cells of
        # every copy stay below num_routed; copies per row divide 4 (one digest word per copy)
        self.ra_stride = 2 + (1 << cap_height) + cap_height
        self.ra_copies = next(c for c in (4, 2, 1) if (c - 1) * self.ra_stride + 2 + (1 << cap_height) <= num_routed)
        self.ra_rows = 4 // self.ra_copies
        self.n_leaf_rows = 0 if leaf_len <= 4 else -(-leaf_len // 8)
        self.n_cap = 1 << cap_height
        self.n_pi = 4 * self.n_cap + n_paths * (2 + leaf_len)
        self.n_pi_rows = -(-self.n_pi // 8)
        self._layout_rows(min_log_n)
        self._programs()
        self._wiring()

    # ---- rows ----
    def _layout_rows(self, min_log_n):
        r = 2                                                   # row 0 PublicInput, row 1 Constant (0)
        self.pi_row, self.const_row = 0, 1
        self.bs_row, self.ra_row, self.leaf_row, self.path_row = [], [], [], []
        for _ in range(self.n_paths):
            self.bs_row.append(r); r += 1
            self.ra_row.append(list(range(r, r + self.ra_rows))); r += self.ra_rows
            self.leaf_row.append(list(range(r, r + self.n_leaf_rows))); r += self.n_leaf_rows
            self.path_row.append(list(range(r, r + self.height))); r += self.height
        self.chain_row = list(range(r, r + self.n_pi_rows))
        r += self.n_pi_rows
        self.rows_used = r
        self.log_n = max(min_log_n, (r - 1).bit_length())
        self.n = 1 << self.log_n
        gate = np.full(self.n, NOOP, dtype=np.int64)
        gate[self.pi_row], gate[self.const_row] = PUBLIC_INPUT, CONSTANT
        for k in range(self.n_paths):
            gate[self.bs_row[k]] = BASE_SUM
            gate[self.ra_row[k]] = RANDOM_ACCESS
            gate[self.leaf_row[k] + self.path_row[k]] = POSEIDON_SWAP
        gate[self.chain_row] = POSEIDON_SWAP
        self.gate = gate

    def _programs(self):
        pr, gates = _Prog(), []
        # group 0 (selector column 0): Noop, PublicInput, Constant, BaseSum -- filter degree 3 + 1, gate degree <= 2
        gates.append((0, NOOP, 0, 4, len(pr.words), 0))
        off, c0 = len(pr.words), pr.count
        for i in range(4):
            pr.constraint([(1, [(_W, i)]), (-1, [(_PIH, i)])])
        gates.append((0, PUBLIC_INPUT, 0, 4, off, pr.count - c0))
        off, c0 = len(pr.words), pr.count
        pr.constraint([(1, [(_W, 0)]), (-1, [(_K, _C0)])])
        gates.append((0, CONSTANT, 0, 4, off, pr.count - c0))
        off, c0 = len(pr.words), pr.count
        pr.constraint([(1 << i, [(_W, 1 + i)]) for i in range(self.height)] + [(-1, [(_W, 0)])])
        for i in range(self.height):
            pr.constraint([(1, [(_W, 1 + i), (_W, 1 + i)]), (-1, [(_W, 1 + i)])])
        gates.append((0, BASE_SUM, 0, 4, off, pr.count - c0))
        # group 1 (selector column 1): RandomAccess -- filter degree 1, gate degree cap_height + 1
        off, c0 = len(pr.words), pr.count
        ch, ln = self.cap_height, self.n_cap
        for cp in range(self.ra_copies):
            b = self.ra_stride * cp
            bits = [(_W, b + 2 + ln + l) for l in range(ch)]
            for x in bits:
                pr.constraint([(1, [x, x]), (-1, [x])])
            pr.constraint([(1 << l, [bits[l]]) for l in range(ch)] + [(-1, [(_W, b)])])
            # the folded list: sum_j item_j prod_l (bit_l if bit l of j else 1 - bit_l), expanded into monomials
            monos = []
            for j in range(ln):
                terms = [(1, [(_W, b + 2 + j)])]
                for l in range(ch):
                    if (j >> l) & 1:
                        terms = [(c, f + [bits[l]]) for c, f in terms]
                    else:
                        terms = [t for c, f in terms for t in ((c, f), (-c, f + [bits[l]]))]
                monos += terms
            pr.constraint(monos + [(-1, [(_W, b + 1)])])
        gates.append((1, RANDOM_ACCESS, 4, 5, off, pr.count - c0))
        # group 2 (selector column 2): PoseidonSwap alone -- filter degree 1, gate degree 7
        off, c0 = len(pr.words), pr.count
        _swap_gate_into(pr, self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox)
        gates.append((2, POSEIDON_SWAP, 5, 6, off, pr.count - c0))
        self.gates, self.programs = gates, np.array(pr.words, dtype=np.int64)

    # ---- copy cycles and the level schedule ----
    def _wiring(self):
        n = self.n
        cell = lambda w, r: w * n + r
        cycles = []                     # lists of cells; every cell at most once
        copies = []                     # (level of the source, src cell, dst cell)
        zero_src = cell(0, self.const_row)
        zero = [zero_src]
        self.pi_cells = [None] * self.n_pi             # the PI chain's input cell of public input t
        pi_cycle = [[] for _ in range(self.n_pi)]
        # PI chain: row j absorbs pis[8 j .. 8 j + len_j)
        for j, r in enumerate(self.chain_row):
            ln = min(8, self.n_pi - 8 * j)
            for t in range(ln):
                self.pi_cells[8 * j + t] = cell(self.s_in + t, r)
                pi_cycle[8 * j + t].append(cell(self.s_in + t, r))
            for t in range(ln, 12):
                if j == 0:
                    zero.append(cell(self.s_in + t, r))
                else:
                    copies.append((j, cell(self.s_out + t, self.chain_row[j - 1]), cell(self.s_in + t, r)))
            zero.append(cell(self.s_swap, r))
        # the final digest <-> the PublicInput gate's wires (both generated: no copy)
        for t in range(4):
            cycles.append([cell(self.s_out + t, self.chain_row[-1]), cell(t, self.pi_row)])
        cap_base = 0
        for k in range(self.n_paths):
            base = 4 * self.n_cap + k * (2 + self.leaf_len)
            hi_t, lo_t, leaf_t = base, base + 1, base + 2
            # index bits
            pi_cycle[lo_t].append(cell(0, self.bs_row[k]))
            # cap selection: copy q = digest word q
            for q in range(4):
                r = self.ra_row[k][q // self.ra_copies]
                b = self.ra_stride * (q % self.ra_copies)
                pi_cycle[hi_t].append(cell(b, r))
                for j in range(self.n_cap):
                    pi_cycle[cap_base + 4 * j + q].append(cell(b + 2 + j, r))
                cycles.append([cell(self.s_out + q, self.path_row[k][-1]), cell(b + 1, r)])      # root word = claimed word
            # leaf hash (hash_or_noop)
            for c, r in enumerate(self.leaf_row[k]):
                ln = min(8, self.leaf_len - 8 * c)
                for t in range(ln):
                    pi_cycle[leaf_t + 8 * c + t].append(cell(self.s_in + t, r))
                for t in range(ln, 12):
                    if c == 0:
                        zero.append(cell(self.s_in + t, r))
                    else:
                        copies.append((c, cell(self.s_out + t, self.leaf_row[k][c - 1]), cell(self.s_in + t, r)))
                zero.append(cell(self.s_swap, r))
            # the path
            for l, r in enumerate(self.path_row[k]):
                for t in range(4):
                    if l > 0:
                        copies.append((self.n_leaf_rows + l, cell(self.s_out + t, self.path_row[k][l - 1]), cell(self.s_in + t, r)))
                    elif self.n_leaf_rows:
                        copies.append((self.n_leaf_rows, cell(self.s_out + t, self.leaf_row[k][-1]), cell(self.s_in + t, r)))
                    elif t < self.leaf_len:
                        pi_cycle[leaf_t + t].append(cell(self.s_in + t, r))
                    else:
                        zero.append(cell(self.s_in + t, r))
                for t in range(8, 12):
                    zero.append(cell(self.s_in + t, r))
                copies.append((0, cell(1 + l, self.bs_row[k]), cell(self.s_swap, r)))         # swap = bit l of the low index
        copies += [(0, zero_src, d) for d in zero[1:]]
        cycles.append(zero)
        cycles += [c for c in pi_cycle if len(c) > 1]
        cycles += [[s, d] for _, s, d in copies if s != zero_src]
        self.pi_cycle = pi_cycle
        self.cycles = cycles
        # levels: 0 = the rows that read public inputs only (PublicInput, Constant, BaseSum, RandomAccess), then 1 + j = link j of every
        # hash chain (the PI chain, the leaf hashes followed by the path)
        row_level = np.full(self.n, -1, dtype=np.int64)
        row_level[[self.pi_row, self.const_row]] = 0
        for k in range(self.n_paths):
            row_level[self.bs_row[k]] = 0
            row_level[self.ra_row[k]] = 0
            for c, r in enumerate(self.leaf_row[k] + self.path_row[k]):
                row_level[r] = 1 + c
        for j, r in enumerate(self.chain_row):
            row_level[r] = 1 + j
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
        # the input cells the partial witness sets: every cell of a cycle that no generator writes, and the siblings
        self.sibling_cells = [[[cell(self.s_in + 4 + t, r) for t in range(4)] for r in self.path_row[k]] for k in range(self.n_paths)]

    # ---- the public face ----
    def circuit(self):
        """the circuit dict of tools/plonk_synth.circuit(): num_wires, num_routed, num_constants, num_selectors, gates, programs"""
        return {"num_wires": self.num_wires, "num_routed": self.num_routed, "num_constants": 4, "num_selectors": 3, "gates": list(self.gates),
                "programs": self.programs, "num_gate_constraints": max(g[5] for g in self.gates), "gate_names": GATE_NAMES}

    def generators(self):
        """[(kind, selector_index, row, p0 .. p4)] (include/sipp_hip.h sipp_plonk_generator)"""
        return [(GEN_PUBLIC_INPUT, 0, PUBLIC_INPUT, 0, 0, 0, 0, 0),
                (GEN_CONSTANT, 0, CONSTANT, 1, _C0, 0, 0, 0),
                (GEN_BASE_SPLIT, 0, BASE_SUM, self.height, 1, 0, 0, 0),
                (GEN_RANDOM_ACCESS, 1, RANDOM_ACCESS, self.ra_copies, self.ra_stride, self.cap_height, 0, 0),
                (GEN_POSEIDON_SWAP, 2, POSEIDON_SWAP, self.s_in, self.s_out, self.s_sbox, self.s_swap, self.s_delta)]

    def schedule(self):
        """the level schedule of sipp_plonk_generate_witness_levels: n_levels, row_level, rows, level_offsets, copy_src / copy_dst
        (cell = wire * N + row), copy_offsets"""
        return self._schedule

    def constants_sigmas(self):
        """[4 + num_routed][N]: the three selector columns, the Constant gate's value (0), the sigmas of the copy cycles (k_i = 7^i)"""
        n, R = self.n, self.num_routed
        groups = ((0, 4), (4, 5), (5, 6))
        sels = [np.where((self.gate >= lo) & (self.gate < hi), self.gate, UNUSED).astype(np.uint64) for lo, hi in groups]
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
        return np.ascontiguousarray(np.concatenate([np.stack(sels + [np.zeros(n, dtype=np.uint64)]), sig]).astype(np.uint64))

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
        pis = self.public_inputs(cap, idx, leaves)
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        flat = w.reshape(-1)
        for t, cyc in enumerate(self.pi_cycle):
            flat[np.asarray(cyc, dtype=np.int64)] = np.uint64(pis[t] % P)
        for k in range(self.n_paths):
            for l in range(self.height):
                flat[np.asarray(self.sibling_cells[k][l], dtype=np.int64)] = siblings[k, l]
        return w


class MerkleOpeningProver:
    """MerkleOpeningCircuit through the library's CircuitData (sipp_circuit_build / _prove / _verify): the constants_sigmas commitment and
    the schedule go to the device once; prove(cap, idx, leaves, siblings) generates the witness there and returns the flat proof."""

    def __init__(self, ctx, leaf_len, height, cap_height, n_paths, fri=None, params=None, digest=None, min_log_n=10):
        from . import _lib
        self.circ = MerkleOpeningCircuit(leaf_len, height, cap_height, n_paths, min_log_n=min_log_n)
        c = self.circ
        self.params = params if params is not None else _lib.PlonkParams(c.num_routed, 8, 2)
        self.fri = fri if fri is not None else fri_params(c.log_n)
        self.circuit = self.circ.circuit()
        self._pc = _lib.PlonkCircuit.from_dict(self.circuit)
        self.data = _lib.CircuitData(ctx, c.log_n, self.params, self.fri, self._pc, c.constants_sigmas(), c.generators(), sched=c.schedule(),
                                     digest=digest)
        self.cap, self.digest = self.data.cap, self.data.digest

    def prove(self, cap, idx, leaves, siblings):
        c = self.circ
        return self.data.prove(c.partial_witness(cap, idx, leaves, siblings), c.public_inputs(cap, idx, leaves))

    def verify(self, proof):
        """-> (status, refusing stage): (0, 0) = accepted"""
        return self.data.verify(proof)

    def close(self):
        self.data.close()


def fri_params(log_n, rate_bits=3, cap_height=4, pow_bits=16, num_queries=28, arity_bits=4, final_poly_bits=5):
    """sipp_fri_params with plonky2's ConstantArityBits(arity_bits, final_poly_bits) reduction for degree_bits = log_n"""
    from . import _lib
    p = _lib.FriParams()
    p.rate_bits, p.cap_height, p.pow_bits, p.num_queries, p.pow_rule, p.hiding = rate_bits, cap_height, pow_bits, num_queries, 0, 0
    d, k = log_n, 0
    while d > final_poly_bits and d + rate_bits - arity_bits >= cap_height and d >= arity_bits and k < 32:
        p.arity_bits[k] = arity_bits
        d -= arity_bits
        k += 1
    p.n_rounds = k
    return p
