"""FRI's initial combination in the outer circuit: plonky2's ReducingGate and ReducingExtensionGate as gate programs, the quotient row of
div_add_extension (an ArithmeticExtension row whose multiplicand a generator fills), and a circuit that proves what fri_combine_initial
does for every query (fri/recursive_verifier.rs, recalled): the step between the Merkle paths (sipp_amd/merkle.py) and the fold chains
(sipp_amd/fri_fold.py).

  reducing_gate          2 K constraints:  acc_i - (acc_(i-1) alpha + c_i)  over F[X]/(X^2 - W), limb by limb; base-field coefficients
  reducing_ext_gate      the same with extension coefficients
  FriInitialCircuit      the gate set, the rows, the copy cycles (sigmas), the generators and the level schedule of the statement
                         "every query's leaf values and the claimed openings combine into the value that enters its first fold"
  FriInitialProver       the circuit through the library's CircuitData: built once, then prove(alpha, points, opened, queries) / verify

Layouts are the generators' (include/sipp_hip.h, SIPP_GEN_REDUCING / _REDUCING_EXT / _QUOTIENT_EXT).  The quotient row has
arithmetic_ext_gate's program under a gate index of its own: its selector value picks the generator that writes the multiplicand from the
output instead of the output from the multiplicand.

Statement layout.  Public inputs = alpha (ext) || per batch (the point (ext), the opened values (ext each)) || per query (x_index, the
n_columns leaf values, the value `old` entering the first fold (ext)).  They are hashed in circuit by the swap-0 Poseidon chain and tied
to the PublicInput gate as in sipp_amd/merkle.py.  Once per proof and batch: a chain of ReducingExt rows gives sum_j alpha^j opened_j;
ArithmeticExt rows give alpha^len by square and multiply on the build-time length.  Per query: a BaseSum row (1-bit limbs) splits
x_index; an Exponentiation row raises omega_M to rev(x_index); an arithmetic op multiplies by the coset generator 7: x (as FriFoldCircuit
has it).  Per batch: a chain of Reducing rows over the batch's leaf values; two arithmetic ops for the numerator acc_x - acc_o and the
denominator (x, 0) - point; the quotient row; total <- total alpha^len + quotient.  Last: old = total (x, 0), tied to its public input.

Chunking.  A chain takes its coefficients highest index first (the result is sum_j alpha^j v_j), K to a row; the FIRST row carries the
len mod K remainder behind leading zero coefficients, whose cells are tied to the zero cell: the accumulator stays 0 through them.

Out of scope: joining this circuit with the Merkle and fold circuits into one query round; the proof of work; empty batches; salt
columns (they are not opened); blinding.

numpy only; imports nothing from the test oracle."""
import numpy as np

from .fri_fold import (COSET_GEN, EXT_W, GEN_ARITHMETIC_EXT, GEN_EXPONENTIATION, _arithmetic_ext_into, _Cells, _exponentiation_into, _words)
from .merkle import (GEN_BASE_SPLIT, GEN_CONSTANT, GEN_POSEIDON_SWAP, GEN_PUBLIC_INPUT, P, SWAP_LAYOUT, UNUSED, _K, _PIH, _Prog, _W, _gl_mul,
                     _powers, _root_of_unity, _swap_gate_into, fri_params)

# include/sipp_hip.h SIPP_GEN_*
GEN_REDUCING, GEN_REDUCING_EXT, GEN_QUOTIENT_EXT = 7, 13, 14
GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "ArithmeticExt", "Reducing", "ReducingExt", "QuotientExt", "Exponentiation",
              "PoseidonSwap"]
NOOP, PUBLIC_INPUT, CONSTANT, BASE_SUM, ARITHMETIC_EXT, REDUCING, REDUCING_EXT, QUOTIENT_EXT, EXPONENTIATION, POSEIDON_SWAP = range(10)
# selector groups [lo, hi): filter degree (hi - lo - 1) + 1, and with the gate's degree at most 8
GROUPS = ((0, 5), (5, 9), (9, 10))
_C0, _C1 = 3, 4                                 # the two constant columns behind the three selector columns


def reducing_layout(K, ext):
    """wire positions of SIPP_GEN_REDUCING (ext = False) / SIPP_GEN_REDUCING_EXT: coefficient i at coeffs + (2 if ext else 1) i"""
    accs = 4 + (2 if ext else 1) * K
    return {"alpha": 0, "old": 2, "coeffs": 4, "accs": accs, "last": accs + 2 * (K - 1), "num_wires": accs + 2 * K}


def _reducing_into(pr, K, W, ext):
    lay = reducing_layout(K, ext)
    al0, al1 = (_W, 0), (_W, 1)
    for i in range(K):
        prev = lay["accs"] + 2 * (i - 1) if i else lay["old"]
        p0, p1, a = (_W, prev), (_W, prev + 1), lay["accs"] + 2 * i
        c = lay["coeffs"] + (2 if ext else 1) * i
        pr.constraint([(1, [(_W, a)]), (-1, [p0, al0]), (-W, [p1, al1]), (-1, [(_W, c)])])
        pr.constraint([(1, [(_W, a + 1)]), (-1, [p0, al1]), (-1, [p1, al0])] + ([(-1, [(_W, c + 1)])] if ext else []))


def reducing_gate(K, W=EXT_W):
    """ReducingGate: per coefficient the two limbs of  acc_i - (acc_(i-1) alpha + c_i),  c_i in the base field; degree 2"""
    assert K >= 1 and W % P
    pr, words = _words(_reducing_into, K, W, False)
    assert pr.count == 2 * K
    return words


def reducing_ext_gate(K, W=EXT_W):
    """ReducingExtensionGate: per coefficient the two limbs of  acc_i - (acc_(i-1) alpha + c_i),  c_i in the extension; degree 2"""
    assert K >= 1 and W % P
    pr, words = _words(_reducing_into, K, W, True)
    assert pr.count == 2 * K
    return words


def _pi(t):
    return ("pi", t)


class FriInitialCircuit:
    """The circuit of fri_combine_initial for n_queries queries of a FRI opening proof over an LDE of 2^log_m points.  A query opens
    n_columns leaf values (the unsalted columns of every oracle, concatenated); batch b combines the columns batches[b] (indices into
    that row, in the order of the batch's opened values) at its point.  Cells are wire * N + row."""

    def __init__(self, log_m, n_columns, batches, n_queries, num_wires=135, num_routed=80, k_base=None, k_ext=None, min_log_n=10):
        batches = [[int(c) for c in b] for b in batches]
        assert 1 <= log_m <= 64 and n_columns >= 1 and n_queries >= 1 and batches
        assert all(len(b) >= 1 for b in batches), "an empty batch is out of scope"
        assert all(0 <= c < n_columns for b in batches for c in b)
        assert 2 + 2 * log_m <= num_wires and 2 + log_m <= num_routed and num_wires >= 135
        # the largest K whose coefficient and last-accumulator cells are routed
        k_base = (num_routed - 4) // 3 if k_base is None else k_base
        k_ext = (num_routed - 4) // 4 if k_ext is None else k_ext
        assert k_base >= 1 and 3 * k_base + 4 <= num_routed and k_ext >= 1 and 4 * k_ext + 4 <= num_routed
        self.log_m, self.n_columns, self.batches, self.n_queries = log_m, n_columns, batches, n_queries
        self.num_wires, self.num_routed, self.k_base, self.k_ext = num_wires, num_routed, k_base, k_ext
        lay = SWAP_LAYOUT
        self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox = lay["in_"], lay["out"], lay["swap"], lay["delta"], lay["sbox"]
        self.omega_m = _root_of_unity(log_m)
        self.pi_batch, t = [], 2
        for b in batches:
            self.pi_batch.append(t)
            t += 2 + 2 * len(b)
        self.pi_queries = t
        self.n_pi = t + n_queries * (3 + n_columns)
        self.n_pi_rows = -(-self.n_pi // 8)
        self._programs()
        self._build(min_log_n)

    # public-input positions
    def pi_point(self, b, l):
        return self.pi_batch[b] + l

    def pi_opened(self, b, j, l):
        return self.pi_batch[b] + 2 + 2 * j + l

    def pi_query(self, q):
        return self.pi_queries + q * (3 + self.n_columns)

    def pi_leaf(self, q, c):
        return self.pi_query(q) + 1 + c

    def pi_old(self, q, l):
        return self.pi_query(q) + 1 + self.n_columns + l

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
        add(REDUCING, 1, lambda: _reducing_into(pr, self.k_base, EXT_W, False))
        add(REDUCING_EXT, 1, lambda: _reducing_into(pr, self.k_ext, EXT_W, True))
        add(QUOTIENT_EXT, 1, lambda: _arithmetic_ext_into(pr, 1, _C0, _C1, EXT_W))
        add(EXPONENTIATION, 1, lambda: _exponentiation_into(pr, self.log_m))
        add(POSEIDON_SWAP, 2, lambda: _swap_gate_into(pr, self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox))
        self.gates, self.programs = gates, np.array(pr.words, dtype=np.int64)
        self.gate_degree = [0, 1, 1, 2, 3, 2, 2, 3, 4, 7]
        for (grp, idx, lo, hi, _, _), deg in zip(gates, self.gate_degree):
            assert (hi - lo - 1) + 1 + deg <= 8, GATE_NAMES[idx]

    # ---- rows, copy cycles and the level schedule: cells are (wire, row) until N is known ----
    def _build(self, min_log_n):
        rows, level = [], {}                            # row -> (gate, c0, c1); row -> level
        uf, copies = _Cells(), []                       # copies: (level of the source, src cell, dst cell)
        pi_cells = [None] * self.n_pi                   # one cell of public input t: every cell of its cycle takes its value

        def new_row(gate, c0=0, c1=0):
            rows.append((gate, c0 % P, c1 % P))
            return len(rows) - 1

        def pi(t, c):
            if pi_cells[t] is None:
                pi_cells[t] = c
            uf.tie(pi_cells[t], c)

        def place(row, feeds):
            """feeds = [(wire, source)]: a source is ("pi", t) or ("cell", cell, level of its row); the row runs one level behind its
            latest computed source"""
            lv = max([s[2] + 1 for _, s in feeds if s[0] == "cell"] or [0])
            for wire, s in feeds:
                if s[0] == "pi":
                    pi(s[1], (wire, row))
                else:
                    uf.tie(s[1], (wire, row))
                    copies.append((s[2], s[1], (wire, row)))
            level[row] = lv

        def out(row, wire):
            return ("cell", (wire, row), level[row])

        def constant(v):
            r = new_row(CONSTANT, v)
            place(r, [])
            return r, out(r, 0)

        def arith(a, m, c, c0, c1):
            """c0 a m + c1 c"""
            r = new_row(ARITHMETIC_EXT, c0, c1)
            place(r, [(0, a[0]), (1, a[1]), (2, m[0]), (3, m[1]), (4, c[0]), (5, c[1])])
            return r, (out(r, 6), out(r, 7))

        self.pi_row = new_row(PUBLIC_INPUT)
        place(self.pi_row, [])
        self.zero_row, zero = constant(0)
        self.one_row, one = constant(1)
        self.omega_row, omega = constant(self.omega_m)
        ZERO, ONE, alpha = (zero, zero), (one, zero), (_pi(0), _pi(1))

        def chain(ext, coeffs):
            """sum_j alpha^j coeffs[j] by rows of K coefficients, highest index first; -> (the rows, the last accumulator)"""
            K, gate = (self.k_ext, REDUCING_EXT) if ext else (self.k_base, REDUCING)
            lay = reducing_layout(K, ext)
            seq = [None] * (-len(coeffs) % K) + list(reversed(coeffs))
            acc, used = ZERO, []
            for at in range(0, len(seq), K):
                r = new_row(gate)
                feeds = [(0, alpha[0]), (1, alpha[1]), (2, acc[0]), (3, acc[1])]
                for j, v in enumerate(seq[at:at + K]):
                    if ext:
                        v = ZERO if v is None else v
                        feeds += [(lay["coeffs"] + 2 * j, v[0]), (lay["coeffs"] + 2 * j + 1, v[1])]
                    else:
                        feeds.append((lay["coeffs"] + j, zero if v is None else v))
                place(r, feeds)
                acc = (out(r, lay["last"]), out(r, lay["last"] + 1))
                used.append(r)
            return used, acc

        # once per proof and batch: the reduced openings, alpha^len
        self.opened_row, self.power_row, acc_o, alpha_len = [], [], [], []
        for b, cols in enumerate(self.batches):
            used, acc = chain(True, [(_pi(self.pi_opened(b, j, 0)), _pi(self.pi_opened(b, j, 1))) for j in range(len(cols))])
            self.opened_row.append(used)
            acc_o.append(acc)
            pw, used = alpha, []
            for bit in bin(len(cols))[3:]:                                       # below the top bit: square, multiply on a 1
                r, pw = arith(pw, pw, ZERO, 1, 0)
                used.append(r)
                if bit == "1":
                    r, pw = arith(pw, alpha, ZERO, 1, 0)
                    used.append(r)
            self.power_row.append(used)
            alpha_len.append(pw)
        # per query
        M = self.log_m
        self.bs_row, self.exp0_row, self.x_row, self.leaf_row, self.num_row, self.den_row, self.quot_row, self.total_row, self.old_row = (
            [], [], [], [], [], [], [], [], [])
        for q in range(self.n_queries):
            bs = new_row(BASE_SUM)
            place(bs, [(0, _pi(self.pi_query(q)))])
            # omega_M ^ rev(x_index): exponent bit j = index bit M - 1 - j
            e0 = new_row(EXPONENTIATION)
            place(e0, [(0, omega)] + [(1 + j, out(bs, 1 + (M - 1 - j))) for j in range(M)])
            # x = 7 (omega_M ^ rev, 0): the c operand
            xr, x = arith(ZERO, ZERO, (out(e0, 1 + M), zero), 0, COSET_GEN)
            self.bs_row.append(bs); self.exp0_row.append(e0); self.x_row.append(xr)
            total = ZERO
            lf, nm, dn, qt, tt = [], [], [], [], []
            for b, cols in enumerate(self.batches):
                used, acc_x = chain(False, [_pi(self.pi_leaf(q, c)) for c in cols])
                lf.append(used)
                r, num = arith(acc_x, ONE, acc_o[b], 1, -1)                      # acc_x - acc_o
                nm.append(r)
                r, den = arith(x, ONE, (_pi(self.pi_point(b, 0)), _pi(self.pi_point(b, 1))), 1, -1)      # (x, 0) - point
                dn.append(r)
                # the quotient: out = a m, the generator fills m = out inv(a)
                r = new_row(QUOTIENT_EXT, 1, 0)
                place(r, [(0, den[0]), (1, den[1]), (4, zero), (5, zero), (6, num[0]), (7, num[1])])
                qt.append(r)
                r, total = arith(total, alpha_len[b], (out(r, 2), out(r, 3)), 1, 1)
                tt.append(r)
            r, old = arith(total, x, ZERO, 1, 0)
            for l in range(2):
                pi(self.pi_old(q, l), old[l][1])
            self.leaf_row.append(lf); self.num_row.append(nm); self.den_row.append(dn); self.quot_row.append(qt); self.total_row.append(tt)
            self.old_row.append(r)
        # the PI chain: row j absorbs pis[8 j .. 8 j + len_j)
        self.chain_row = []
        for j in range(self.n_pi_rows):
            r = new_row(POSEIDON_SWAP)
            ln = min(8, self.n_pi - 8 * j)
            feeds = [(self.s_in + t, _pi(8 * j + t)) for t in range(ln)]
            feeds += [(self.s_in + t, out(self.chain_row[-1], self.s_out + t) if j else zero) for t in range(ln, 12)]
            place(r, feeds + [(self.s_swap, zero)])
            self.chain_row.append(r)
        for t in range(4):
            uf.tie((self.s_out + t, self.chain_row[-1]), (t, self.pi_row))
        # ---- N is known: cells become wire * N + row ----
        self.rows_used = len(rows)
        self.log_n = max(min_log_n, (len(rows) - 1).bit_length())
        n = self.n = 1 << self.log_n
        self.gate = np.full(n, NOOP, dtype=np.int64)
        self.c0, self.c1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        for r, (g, c0, c1) in enumerate(rows):
            self.gate[r], self.c0[r], self.c1[r] = g, c0, c1
        cell = lambda c: c[0] * n + c[1]
        groups = uf.groups()
        self.cycles = [sorted(cell(c) for c in g) for g in groups.values() if len(g) > 1]
        self.pi_cells = [cell(c) for c in pi_cells]
        self.pi_cycle = [sorted(cell(x) for x in groups[uf.find(c)]) for c in pi_cells]
        row_level = np.full(n, -1, dtype=np.int64)
        for r, lv in level.items():
            row_level[r] = lv
        assert (row_level[:len(rows)] >= 0).all()
        self.row_level = row_level
        self.n_levels = int(row_level.max()) + 1
        lev = np.array([c[0] for c in copies], dtype=np.int64)
        src = np.array([cell(c[1]) for c in copies], dtype=np.uint64)
        dst = np.array([cell(c[2]) for c in copies], dtype=np.uint64)
        o = np.argsort(lev, kind="stable")
        lev, src, dst = lev[o], src[o], dst[o]
        sched_rows = np.flatnonzero(row_level >= 0)
        order = sched_rows[np.lexsort((sched_rows, self.gate[sched_rows], row_level[sched_rows]))].astype(np.uint32)
        self._schedule = {"n_levels": self.n_levels, "row_level": row_level, "rows": order,
                          "level_offsets": np.searchsorted(row_level[order], np.arange(self.n_levels + 1)).astype(np.uint32),
                          "copy_src": src, "copy_dst": dst,
                          "copy_offsets": np.searchsorted(lev, np.arange(self.n_levels + 1)).astype(np.uint32)}

    # ---- the public face ----
    def circuit(self):
        """the circuit dict of tools/plonk_synth.circuit(): num_wires, num_routed, num_constants, num_selectors, gates, programs"""
        return {"num_wires": self.num_wires, "num_routed": self.num_routed, "num_constants": 5, "num_selectors": 3, "gates": list(self.gates),
                "programs": self.programs, "num_gate_constraints": max(g[5] for g in self.gates), "gate_names": GATE_NAMES}

    def generators(self):
        """[(kind, selector_index, row, p0 .. p4)] (include/sipp_hip.h sipp_plonk_generator)"""
        return [(GEN_PUBLIC_INPUT, 0, PUBLIC_INPUT, 0, 0, 0, 0, 0),
                (GEN_CONSTANT, 0, CONSTANT, 1, _C0, 0, 0, 0),
                (GEN_BASE_SPLIT, 0, BASE_SUM, self.log_m, 1, 0, 0, 0),
                (GEN_ARITHMETIC_EXT, 0, ARITHMETIC_EXT, 1, _C0, _C1, EXT_W, 0),
                (GEN_REDUCING, 1, REDUCING, self.k_base, EXT_W, 0, 0, 0),
                (GEN_REDUCING_EXT, 1, REDUCING_EXT, self.k_ext, EXT_W, 0, 0, 0),
                (GEN_QUOTIENT_EXT, 1, QUOTIENT_EXT, 1, _C0, _C1, EXT_W, 0),
                (GEN_EXPONENTIATION, 1, EXPONENTIATION, self.log_m, 0, 0, 0, 0),
                (GEN_POSEIDON_SWAP, 2, POSEIDON_SWAP, self.s_in, self.s_out, self.s_sbox, self.s_swap, self.s_delta)]

    def schedule(self):
        """the level schedule of sipp_plonk_generate_witness_levels"""
        return self._schedule

    def constants_sigmas(self):
        """[5 + num_routed][N]: the three selector columns, the two constant columns, the sigmas of the copy cycles (k_i = 7^i)"""
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

    def _check(self, alpha, points, opened, queries):
        ext = lambda v: (int(v[0]) % P, int(v[1]) % P)
        assert len(points) == len(self.batches) == len(opened) and len(queries) == self.n_queries
        opened = [[ext(v) for v in vals] for vals in opened]
        assert all(len(vals) == len(b) for vals, b in zip(opened, self.batches))
        out = []
        for x_index, leaves, old in queries:
            x_index = int(x_index)
            assert 0 <= x_index < (1 << self.log_m) and len(leaves) == self.n_columns
            out.append((x_index, [int(v) % P for v in leaves], ext(old)))
        return ext(alpha), [ext(p) for p in points], opened, out

    def public_inputs(self, alpha, points, opened, queries):
        """alpha || per batch (point, opened values) || per query (x_index, leaf values, old), as ints; ext values as (c0, c1) pairs"""
        alpha, points, opened, queries = self._check(alpha, points, opened, queries)
        out = list(alpha)
        for pt, vals in zip(points, opened):
            out += list(pt) + [l for v in vals for l in v]
        for x_index, leaves, old in queries:
            out += [x_index] + leaves + list(old)
        assert len(out) == self.n_pi
        return out

    def partial_witness(self, alpha, points, opened, queries):
        """[num_wires][N] with the INPUT cells set: every cell on a cycle of a public input; everything else 0"""
        pis = self.public_inputs(alpha, points, opened, queries)
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        flat = w.reshape(-1)
        for t, cyc in enumerate(self.pi_cycle):
            flat[np.asarray(cyc, dtype=np.int64)] = np.uint64(pis[t])
        return w


class FriInitialProver:
    """FriInitialCircuit through the library's CircuitData: the constants_sigmas commitment and the schedule go to the device once;
    prove(alpha, points, opened, queries) generates the witness there and returns the flat proof."""

    def __init__(self, ctx, log_m, n_columns, batches, n_queries, fri=None, params=None, digest=None, k_base=None, k_ext=None, min_log_n=10):
        from . import _lib
        self.circ = FriInitialCircuit(log_m, n_columns, batches, n_queries, k_base=k_base, k_ext=k_ext, min_log_n=min_log_n)
        c = self.circ
        self.params = params if params is not None else _lib.PlonkParams(c.num_routed, 8, 2)
        self.fri = fri if fri is not None else fri_params(c.log_n)
        self.circuit = self.circ.circuit()
        self._pc = _lib.PlonkCircuit.from_dict(self.circuit)
        self.data = _lib.CircuitData(ctx, c.log_n, self.params, self.fri, self._pc, c.constants_sigmas(), c.generators(), sched=c.schedule(),
                                     digest=digest)
        self.cap, self.digest = self.data.cap, self.data.digest

    def prove(self, alpha, points, opened, queries):
        c = self.circ
        return self.data.prove(c.partial_witness(alpha, points, opened, queries), c.public_inputs(alpha, points, opened, queries))

    def verify(self, proof):
        """-> (status, refusing stage): (0, 0) = accepted"""
        return self.data.verify(proof)

    def close(self):
        self.data.close()
