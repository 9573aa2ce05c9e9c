"""What the outer prover's statement circuits (sipp_amd/merkle.py, fri_fold.py, fri_initial.py) share: the field and program helpers, the
gate programs more than one of them uses, the builder that turns rows and feeds into what the prover takes, and the prover wrapper.

  _gl_mul, _powers, ...     Goldilocks over numpy (sigmas only); _Prog, the program words of sipp_plonk_circuit; _Cells, the union-find
                            whose sets become the permutation cycles
  GEN_*                     include/sipp_hip.h SIPP_GEN_*
  public_input_into, constant_into, base_sum_into, random_access_into
                            the gate programs without a home of their own; the Poseidon swap gate is sipp_amd/merkle.py's, arithmetic-ext,
                            exponentiation and coset interpolation are sipp_amd/fri_fold.py's, the reducing gates sipp_amd/fri_initial.py's
  CircuitBuilder            the gate registry (selector groups, programs, generators); rows by new_row(); wiring by place(), which ties
                            the cells, schedules the copies and gives every row the level behind its latest computed source, and tie();
                            the public-input Poseidon chain; finish(), which fixes N and makes the cycles and the level schedule.  A
                            circuit is a subclass: it declares its gates, writes its statement as builder calls and finishes.
                            Lookups (include/sipp_hip.h "LOOKUP TABLES"): declare_lookup() names two zero-constraint gates,
                            table() writes the table rows, lookup() / range_check() fill looking rows; the description rides in circuit().
                            declare_lookup(tables=True): several tables told apart by a tag (description word 7), and function tables --
                            function_table(values) is the dense table t -> values[t], function_lookup(table, xs) places looking rows
                            whose y cells SIPP_GEN_LOOKUP fills on the device and returns those cells as sources
                            Blinding (include/sipp_hip.h "ZERO KNOWLEDGE"), off by default: declare_blinding() names a zero-constraint
                            gate whose generator is SIPP_GEN_RANDOM; finish() then appends blinding_counts() rows of it
  blinding_counts           plonky2's rule for the number of blinding rows, as recalled; overridable by keyword
  _Challenger               plonky2's RecursiveChallenger on a builder (sipp_amd/fri_proof.py says how it buffers and duplexes)
  CircuitProver             a built circuit through the library's CircuitData

numpy only; imports nothing from the test oracle."""
import numpy as np

P = 0xFFFFFFFF00000001
PP = np.uint64(P)
M32 = np.uint64(0xFFFFFFFF)
EPS = np.uint64(0xFFFFFFFF)
UNUSED = 0xFFFFFFFF

# include/sipp_hip.h SIPP_GEN_*
GEN_BASE_SPLIT, GEN_CONSTANT, GEN_PUBLIC_INPUT, GEN_RANDOM_ACCESS, GEN_REDUCING, GEN_POSEIDON_SWAP = 2, 3, 4, 6, 7, 9
GEN_ARITHMETIC_EXT, GEN_EXPONENTIATION, GEN_COSET_INTERPOLATION, GEN_REDUCING_EXT, GEN_QUOTIENT_EXT = 10, 11, 12, 13, 14
GEN_BASE_SUM = 15
GEN_POSEIDON_MDS = 16
GEN_LOOKUP = 17
GEN_RANDOM = 18
GEN_U32_ARITHMETIC, GEN_U32_ADD_MANY, GEN_NONNATIVE = 19, 20, 21
# program factor kinds
_W, _K, _PIH = 0, 1, 2
# upstream's PoseidonGate layout (SIPP_GEN_POSEIDON_SWAP): 135 wires
SWAP_LAYOUT = {"in_": 0, "out": 12, "swap": 24, "delta": 25, "sbox": 29}
# the gates every circuit starts with (CircuitBuilder.declare_basic)
NOOP, PUBLIC_INPUT, CONSTANT, BASE_SUM = range(4)


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


def _words(fill, *args):
    pr = _Prog()
    fill(pr, *args)
    return pr, np.array(pr.words, dtype=np.int64)


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


def _fri_shape(fri):
    """(num_queries, the rounds' arity bits) of a sipp_fri_params struct or of a dict with the same names"""
    get = fri.get if isinstance(fri, dict) else lambda k: getattr(fri, k)
    return int(get("num_queries")), [int(a) for a in list(get("arity_bits"))[:int(get("n_rounds"))]]


def blinding_counts(fri, log_n, regular=None, z=None):
    """(regular, z): the blinding rows of a circuit of 2^log_n rows under the FRI parameters `fri` -- plonky2's rule (circuit_builder.rs
    blind_and_pad) as RECALLED, not pinned against upstream; the keywords override either count.  With D = 2 (the extension degree):
        fri_openings = num_queries (1 + D sum_rounds (2^arity_bits - 1) + final_poly_len),  final_poly_len = 2^(log_n - sum arity_bits)
        regular = D + fri_openings      rows whose wires are all random: every wire polynomial is opened at zeta (D values) and at the
                                        queried leaves
        z = 2 D + fri_openings          PAIRS of rows for the permutation argument: Z is opened at zeta and g zeta"""
    D = 2
    q, arity = _fri_shape(fri)
    assert sum(arity) <= log_n
    openings = q * (1 + D * sum((1 << a) - 1 for a in arity) + (1 << (log_n - sum(arity))))
    return (D + openings if regular is None else int(regular)), (2 * D + openings if z is None else int(z))


# ---- the gate programs more than one circuit uses ---------------------------------------------------------------------------------------
def public_input_into(pr):
    for i in range(4):
        pr.constraint([(1, [(_W, i)]), (-1, [(_PIH, i)])])


def constant_into(pr, k0):
    pr.constraint([(1, [(_W, 0)]), (-1, [(_K, k0)])])


def base_sum_into(pr, n_bits):
    """1-bit limbs: the sum, then every limb's booleanity"""
    pr.constraint([(1 << i, [(_W, 1 + i)]) for i in range(n_bits)] + [(-1, [(_W, 0)])])
    for i in range(n_bits):
        pr.constraint([(1, [(_W, 1 + i), (_W, 1 + i)]), (-1, [(_W, 1 + i)])])


def random_access_into(pr, copies, stride, bits):
    """per copy at b = stride cp: index, claimed, 2^bits items, `bits` bits (SIPP_GEN_RANDOM_ACCESS); degree bits + 1"""
    ln = 1 << bits
    for cp in range(copies):
        b = stride * cp
        bit = [(_W, b + 2 + ln + l) for l in range(bits)]
        for x in bit:
            pr.constraint([(1, [x, x]), (-1, [x])])
        pr.constraint([(1 << l, [bit[l]]) for l in range(bits)] + [(-1, [(_W, b)])])
        # the folded list: sum_j item_j prod_l (bit_l if bit l of j else 1 - bit_l), expanded into monomials
        monos = []
        for j in range(ln):
            terms = [(1, [(_W, b + 2 + j)])]
            for l in range(bits):
                if (j >> l) & 1:
                    terms = [(c, f + [bit[l]]) for c, f in terms]
                else:
                    terms = [t for c, f in terms for t in ((c, f), (-c, f + [bit[l]]))]
            monos += terms
        pr.constraint(monos + [(-1, [(_W, b + 1)])])


def pi(t):
    """public input t as a source of place()"""
    return ("pi", t)


def _is_input(s):
    """a public input or a witness input (CircuitBuilder.witness_input): the partial witness sets every cell tied to it"""
    return s[0] in ("pi", "in")


class CircuitBuilder:
    """Gates, rows and wiring of one circuit.  A cell is (wire, row) until finish() knows N, then wire * N + row.  A source of place()
    is pi(t), a witness input or the cell of a row placed before: a row that reads a cell before a generator can have written it does
    not build."""

    def __init__(self, num_wires, num_routed, gate_names, gate_group, n_constants, n_pi):
        """gate_group: the selector group of every gate, ascending; n_constants: the constant columns behind the selector columns"""
        assert len(gate_names) == len(gate_group) and list(gate_group) == sorted(gate_group) and n_constants in (1, 2)
        self.num_wires, self.num_routed, self.gate_names, self.n_pi = num_wires, num_routed, gate_names, n_pi
        self.n_pi_rows = -(-n_pi // 8)
        lay = SWAP_LAYOUT
        self.s_in, self.s_out, self.s_swap, self.s_delta, self.s_sbox = lay["in_"], lay["out"], lay["swap"], lay["delta"], lay["sbox"]
        self.num_selectors = gate_group[-1] + 1
        self.num_constants = self.num_selectors + n_constants
        self.k0, self.k1 = self.num_selectors, self.num_selectors + 1          # the constant columns (k1: if there are two)
        # selector groups [lo, hi): filter degree (hi - lo - 1) + 1, and with the gate's degree at most 8
        self.groups = [(gate_group.index(g), gate_group.index(g) + gate_group.count(g)) for g in range(self.num_selectors)]
        self._group, self._prog, self.gates, self._generators = gate_group, _Prog(), [], []
        self._rows, self._level = [], {}                        # row -> (gate, c0, c1); row -> level
        self._uf, self._copies = _Cells(), []                   # copies: (level of the source, src cell, dst cell)
        self._pi_cells = [None] * n_pi                          # one cell of public input t: every cell of its cycle takes its value
        self._in_cells = []                                     # the same for the witness inputs
        self._lk = None                                         # declare_lookup()'s layout; without one nothing below changes
        self._blind = None                                      # declare_blinding()'s gate and rule; without one nothing below changes
        self.blinding, self.blind_rows = (0, 0), {"regular": [], "pairs": []}

    # ---- gates ----
    def declare(self, index, degree, gen=None, fill=None, *args):
        """the next gate: gen = (kind, p0, ...) is its generator's tuple without (selector, row); fill(pr, *args) writes its program"""
        assert index == len(self.gates)
        group, pr = self._group[index], self._prog
        lo, hi = self.groups[group]
        assert (hi - lo - 1) + 1 + degree <= 8, self.gate_names[index]
        off, cnt = len(pr.words), pr.count
        if fill:
            fill(pr, *args)
        self.gates.append((group, index, lo, hi, off, pr.count - cnt))
        if gen:
            self._generators.append((gen[0], group, index) + (tuple(gen[1:]) + (0,) * 5)[:5])

    def declare_basic(self, n_bits):
        """the gates every circuit starts with: Noop, PublicInput, Constant, BaseSum with n_bits 1-bit limbs"""
        self.declare(NOOP, 0)
        self.declare(PUBLIC_INPUT, 1, (GEN_PUBLIC_INPUT,), public_input_into)
        self.declare(CONSTANT, 1, (GEN_CONSTANT, 1, self.k0), constant_into, self.k0)
        self.declare(BASE_SUM, 2, (GEN_BASE_SPLIT, n_bits, 1), base_sum_into, n_bits)

    # ---- rows and wiring ----
    def new_row(self, gate, c0=0, c1=0):
        self._rows.append((gate, c0 % P, c1 % P))
        return len(self._rows) - 1

    def public_input(self, t, cell):
        if self._pi_cells[t] is None:
            self._pi_cells[t] = cell
        self._uf.tie(self._pi_cells[t], cell)

    def witness_input(self):
        """the next witness input as a source of place(): a value the prover sets and only the constraints bind.  Like a public input
        it has no level: the partial witness sets every cell tied to it"""
        self._in_cells.append(None)
        return ("in", len(self._in_cells) - 1)

    def _input(self, s, cell):
        if s[0] == "pi":
            return self.public_input(s[1], cell)
        if self._in_cells[s[1]] is None:
            self._in_cells[s[1]] = cell
        self._uf.tie(self._in_cells[s[1]], cell)

    def tie(self, a, b):
        """a copy constraint between source a and cell b without a scheduled copy: generators write both, or b is an input cell"""
        if _is_input(a):
            self._input(a, b)
        elif _is_input(b):
            self._input(b, a)
        else:
            self._uf.tie(a, b)

    def place(self, row, feeds=()):
        """feeds = [(wire, source)]: ties every source to its cell of the row and schedules the copies at their sources' levels; the row
        runs one level behind its latest computed source"""
        lv = 0
        for wire, s in feeds:
            if _is_input(s):
                self._input(s, (wire, row))
            else:
                at = self._level[s[1]]
                self._uf.tie(s, (wire, row))
                self._copies.append((at, s, (wire, row)))
                lv = max(lv, at + 1)
        self._level[row] = lv

    def constant(self, v):
        """a Constant row of value v -> (the row, its cell)"""
        r = self.new_row(CONSTANT, v)
        self.place(r)
        return r, (0, r)

    def hash_rows(self, gate, zero, sources):
        """a chain of swap-0 Poseidon rows (hash_n_to_hash_no_pad, overwrite mode) over the sources: every row absorbs the next 8 of them
        or what is left, its other inputs are the outputs of the row before or zero -> the rows; the digest is the last row's out 0 .. 3"""
        rows = []
        for at in range(0, len(sources), 8):
            r = self.new_row(gate)
            feeds = [(self.s_in + t, s) for t, s in enumerate(sources[at:at + 8])]
            feeds += [(self.s_in + t, (self.s_out + t, rows[-1]) if rows else zero) for t in range(len(feeds), 12)]
            self.place(r, feeds + [(self.s_swap, zero)])
            rows.append(r)
        return rows

    def hash_public_inputs(self, gate, zero):
        """the public inputs hashed in circuit: the chain's digest is the PublicInput row's by copy constraint (both generated: no copy),
        which the prover binds to hash_no_pad(public inputs)"""
        self.chain_row = self.hash_rows(gate, zero, [pi(t) for t in range(self.n_pi)])
        for t in range(4):
            self.tie((self.s_out + t, self.chain_row[-1]), (t, self.pi_row))

    # ---- lookups: tables in constant columns, the multiplicities in wires ----
    def declare_lookup(self, table_gate, looking_gate, n_look, n_tab, look_wire0=0, tab_mult0=None, tables=False):
        """table_gate, looking_gate: two gates declared with no constraints (declare(index, 0)) that only mark the table rows and the
        looking rows.  A looking row holds n_look pairs in the routed wires look_wire0 ..; a table row holds n_tab pairs in constant
        columns of their own behind the builder's, its multiplicities in the wires tab_mult0 .. (default: behind the looking wires).
        The constant columns grow by q_look, q_tab and the 2 n_tab table columns.
        tables=True: several tables, told apart by a tag -- two more constant columns behind the table columns (the looking rows' tags,
        the table rows' tags: description word 7); table() may then be called more than once, and the looking gate gets the generator
        SIPP_GEN_LOOKUP, which fills the y cells of function_lookup()'s rows from the row's constants c0 = row0, c1 = T (so the
        builder must have two constant columns); every other looking row has c0 = c1 = 0 and both coordinates fed."""
        assert self._lk is None and 1 <= n_look <= 128 and 1 <= n_tab <= 128
        tab_mult0 = look_wire0 + 2 * n_look if tab_mult0 is None else tab_mult0
        assert look_wire0 + 2 * n_look <= self.num_routed and tab_mult0 + n_tab <= self.num_wires
        k = self.num_constants
        self._lk = {"table_gate": table_gate, "looking_gate": looking_gate, "n_look": n_look, "n_tab": n_tab, "look_wire0": look_wire0,
                    "tab_mult0": tab_mult0, "q_look": k, "q_tab": k + 1, "tab_const0": k + 2, "entries": None, "table_rows": [],
                    "pending": [], "zero": None, "tag_const0": 0, "tables": [], "row_tag": {}}
        self.num_constants = k + 2 + 2 * n_tab
        if tables:
            assert self.num_constants - 2 - 2 * n_tab - self.num_selectors == 2, "function rows keep row0 and T in c0, c1"
            self._lk["tag_const0"] = self.num_constants
            self.num_constants += 2
            self._generators.append((GEN_LOOKUP, self._group[looking_gate], looking_gate, look_wire0, n_look, k + 2, n_tab, self.k0))

    def table(self, entries):
        """the table: (x, y) pairs (a range table: (v, 0)).  Table rows are written here; the slots the last row has left repeat the last
        entry.  -> the entries, as range_check()'s `table` argument; with tables=True a handle (a dict: tag, entries, row0, T) as the
        `table` argument of lookup(), range_check() and function_lookup(), the tables taking the tags 0, 1, 2, ... as they come"""
        lk = self._lk
        assert lk is not None and len(entries) >= 1 and (lk["tag_const0"] or lk["entries"] is None)
        ent = [(int(x) % P, int(y) % P) for x, y in entries]
        handle = {"tag": len(lk["tables"]), "entries": ent, "row0": len(self._rows), "T": len(ent), "pending": [], "dense": False}
        for at in range(0, len(ent), lk["n_tab"]):
            r = self.new_row(lk["table_gate"])
            self.place(r)
            lk["table_rows"].append((r, (ent[at:at + lk["n_tab"]] + [ent[-1]] * lk["n_tab"])[:lk["n_tab"]]))
            lk["row_tag"][r] = handle["tag"]
        lk["tables"].append(handle)
        if not lk["tag_const0"]:
            lk["entries"] = ent
            return ent
        return handle

    def function_table(self, values):
        """the dense table t -> values[t], t < len(values): entry t is (t, values[t]) in table row row0 + t // n_tab, slot t % n_tab,
        which is where SIPP_GEN_LOOKUP reads it.  -> the handle, with row0 and T = len(values)"""
        assert self._lk is not None and self._lk["tag_const0"], "function tables need declare_lookup(tables=True)"
        handle = self.table([(t, v) for t, v in enumerate(values)])
        handle["dense"] = True
        return handle

    def _table(self, table):
        """the handle lookups against `table` gather under: the one table of a circuit without tags, whatever `table` is"""
        lk = self._lk
        assert lk is not None and lk["tables"]
        if not lk["tag_const0"]:
            return lk["tables"][0]
        assert any(table is t for t in lk["tables"]), "with several tables every lookup names its table's handle"
        return table

    def lookup(self, x_source, y_source, table=None):
        """the pair (x, y) must be an entry of the table.  Pairs are gathered per table, n_look to a looking row; a row that stays short
        repeats its first pair (flush_lookups(), which finish() calls)"""
        t = self._table(table)
        t["pending"].append((x_source, y_source))
        if len(t["pending"]) == self._lk["n_look"]:
            self._flush(t)

    def range_check(self, x_source, table=None):
        """x is the first coordinate of an entry (x, 0): a lookup of (x, 0) against a range table"""
        lk = self._lk
        assert lk["tag_const0"] or table is None or table is lk["entries"], "one table a circuit"
        if lk["zero"] is None:
            lk["zero"] = self.constant(0)[1]
        self.lookup(x_source, lk["zero"], table)

    def function_lookup(self, table, x_sources):
        """y = f(x) for every source x, f a function_table(): whole looking rows of up to n_look slots with only the x cells fed (a
        short row repeats its first x), c0 = row0 and c1 = T, so that the looking gate's generator writes the y cells.  A row runs one
        level behind its latest x.  -> the y cells, sources for later rows like any generated cell"""
        lk = self._lk
        assert lk is not None and any(table is t for t in lk["tables"]) and table["dense"]
        n_look, lw, out = lk["n_look"], lk["look_wire0"], []
        for at in range(0, len(x_sources), n_look):
            xs = list(x_sources[at:at + n_look])
            r = self.new_row(lk["looking_gate"], table["row0"], table["T"])
            lk["row_tag"][r] = table["tag"]
            self.place(r, [(lw + 2 * k, s) for k, s in enumerate((xs + [xs[0]] * n_look)[:n_look])])
            out += [(lw + 2 * k + 1, r) for k in range(len(xs))]
        return out

    def _flush(self, t):
        lk = self._lk
        if not t["pending"]:
            return
        pairs = (t["pending"] + [t["pending"][0]] * lk["n_look"])[:lk["n_look"]]
        t["pending"] = []
        r = self.new_row(lk["looking_gate"])
        lk["row_tag"][r] = t["tag"]
        feeds = []
        for k, (xs, ys) in enumerate(pairs):
            feeds += [(lk["look_wire0"] + 2 * k, xs), (lk["look_wire0"] + 2 * k + 1, ys)]
        self.place(r, feeds)

    def flush_lookups(self):
        if self._lk is not None:
            for t in self._lk["tables"]:
                self._flush(t)

    def lookup_description(self):
        """the eight words of include/sipp_hip.h; all zero without a declared lookup"""
        lk = self._lk
        if lk is None:
            return (0,) * 8
        return (lk["q_look"], lk["look_wire0"], lk["n_look"], lk["q_tab"], lk["tab_const0"], lk["tab_mult0"], lk["n_tab"], lk["tag_const0"])

    # ---- blinding rows ----
    def declare_blinding(self, gate, fri_of=None, **counts):
        """gate: a gate of its own, declared with no constraints (declare(index, 0)); it gets the generator SIPP_GEN_RANDOM over every
        wire.  finish() appends the blinding rows behind the circuit's: blinding_counts(fri_of(log_n), log_n, **counts) -- fri_of maps
        the degree bits to the FRI parameters the circuit will be proved under (default: fri_params), counts overrides the rule
        (regular=, z=).  `regular` rows have every wire random; each of `z` PAIRS has a first row like that and a second whose routed
        wires are copies of the first's (scheduled like every copy; its other wires stay random): the sigmas swap the two cells, which
        randomises Z.  Padding rows stay Noop rows of zeros."""
        assert self._blind is None and gate != NOOP and self.gates[gate][5] == 0, "the blinding gate has no constraints and is not Noop"
        self._generators.append((GEN_RANDOM, self._group[gate], gate, 0, self.num_wires, 0, 0, 0))
        self._blind = {"gate": gate, "fri_of": fri_of if fri_of is not None else fri_params, "counts": counts}

    def _blinding_rows(self, min_log_n):
        """plonky2's loop: the counts for the degree the rows reach; if the blinding rows push the table over a power of two, again for
        the larger degree, until they fit"""
        bl, base = self._blind, len(self._rows)
        log_n = max(min_log_n, (base - 1).bit_length())
        while True:
            regular, z = blinding_counts(bl["fri_of"](log_n), log_n, **bl["counts"])
            need = max(min_log_n, (base + regular + 2 * z - 1).bit_length())
            if need <= log_n:
                break
            log_n = need
        g, R = bl["gate"], self.num_routed
        for _ in range(regular):
            r = self.new_row(g)
            self.place(r)
            self.blind_rows["regular"].append(r)
        for _ in range(z):
            a, b = self.new_row(g), self.new_row(g)
            self.place(a)
            self.place(b, [(w, (w, a)) for w in range(R)])
            self.blind_rows["pairs"].append((a, b))
        self.blinding = (regular, z)
        return log_n

    def finish(self, min_log_n):
        """N is known: cells become wire * N + row.  min_log_n: the device prover's FRI takes degree bits 10 .. 24; smaller circuits
        are padded with Noop rows"""
        self.flush_lookups()
        if self._blind is not None:
            min_log_n = self._blinding_rows(min_log_n)
        assert len(self.gates) == len(self.gate_names)
        self.programs = np.array(self._prog.words, dtype=np.int64)
        rows = self._rows
        self.rows_used = len(rows)
        self.log_n = max(min_log_n, (len(rows) - 1).bit_length())
        n = self.n = 1 << self.log_n
        self.gate = np.full(n, NOOP, dtype=np.int64)
        self.c0, self.c1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        for r, (g, c0, c1) in enumerate(rows):
            self.gate[r], self.c0[r], self.c1[r] = g, c0, c1
        cell = lambda c: c[0] * n + c[1]
        groups = self._uf.groups()
        self.cycles = [sorted(cell(c) for c in g) for g in groups.values() if len(g) > 1]
        self.pi_cells = [cell(c) for c in self._pi_cells]
        self.pi_cycle = [sorted(cell(x) for x in groups[self._uf.find(c)]) for c in self._pi_cells]
        self.in_cycle = [sorted(cell(x) for x in groups[self._uf.find(c)]) for c in self._in_cells]
        row_level = np.full(n, -1, dtype=np.int64)
        for r, lv in self._level.items():
            row_level[r] = lv
        assert (row_level[:len(rows)] >= 0).all()
        self.row_level = row_level
        self.n_levels = int(row_level.max()) + 1
        lev = np.array([c[0] for c in self._copies], dtype=np.int64)
        src = np.array([cell(c[1]) for c in self._copies], dtype=np.uint64)
        dst = np.array([cell(c[2]) for c in self._copies], dtype=np.uint64)
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
        out = {"num_wires": self.num_wires, "num_routed": self.num_routed, "num_constants": self.num_constants,
               "num_selectors": self.num_selectors, "gates": list(self.gates), "programs": self.programs,
               "num_gate_constraints": max(g[5] for g in self.gates), "gate_names": self.gate_names}
        if self._lk is not None:
            out["lookup"] = self.lookup_description()
        return out

    def generators(self):
        """[(kind, selector_index, row, p0 .. p4)] (include/sipp_hip.h sipp_plonk_generator)"""
        return list(self._generators)

    def schedule(self):
        """the level schedule of sipp_plonk_generate_witness_levels: n_levels, row_level, rows, level_offsets, copy_src / copy_dst
        (cell = wire * N + row), copy_offsets"""
        return self._schedule

    def constants_sigmas(self):
        """[num_constants + num_routed][N]: the selector columns, the constant columns, the sigmas of the copy cycles (k_i = 7^i)"""
        n, R = self.n, self.num_routed
        sels = [np.where((self.gate >= lo) & (self.gate < hi), self.gate, UNUSED).astype(np.uint64) for lo, hi in self.groups]
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
        consts = [self.c0, self.c1][:self.k_lookup0() - self.num_selectors]
        if self._lk is not None:
            lk = self._lk
            cols = np.zeros((2 + 2 * lk["n_tab"] + (2 if lk["tag_const0"] else 0), n), dtype=np.uint64)
            cols[0] = self.gate == lk["looking_gate"]
            cols[1] = self.gate == lk["table_gate"]
            for r, slots in lk["table_rows"]:
                for k, (x, y) in enumerate(slots):
                    cols[2 + 2 * k][r], cols[3 + 2 * k][r] = x, y
            if lk["tag_const0"]:                      # the looking rows' tags, then the table rows'
                for r, tag in lk["row_tag"].items():
                    cols[2 + 2 * lk["n_tab"] + (self.gate[r] == lk["table_gate"])][r] = tag
            consts = consts + list(cols)
        return np.ascontiguousarray(np.concatenate([np.stack(sels + consts), sig]).astype(np.uint64))

    def k_lookup0(self):
        """the first constant column of the lookup argument (= num_constants without one)"""
        return self.num_constants if self._lk is None else self._lk["q_look"]

    def public_input_witness(self, pis):
        """[num_wires][N] with every cell on a cycle of a public input set (plonky2's PartialWitness), everything else 0: the generators
        and the schedule's copies fill it -> (the array, its flat view)"""
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        flat = w.reshape(-1)
        for t, cyc in enumerate(self.pi_cycle):
            flat[np.asarray(cyc, dtype=np.int64)] = np.uint64(pis[t] % P)
        return w, flat


class _Challenger:
    """plonky2's RecursiveChallenger on a builder: sources in, cells out"""

    def __init__(self, b, gate, zero, state, pending):
        """gate: b's PoseidonSwap gate; state: 12 sources; pending: the buffered input sources"""
        self.b, self.gate, self.zero, self.sponge, self.inbuf, self.outbuf, self.rows = b, gate, zero, list(state), list(pending), [], []

    def _duplex(self):
        b = self.b
        r = b.new_row(self.gate)
        b.place(r, [(b.s_in + t, self.inbuf[t] if t < len(self.inbuf) else self.sponge[t]) for t in range(12)] + [(b.s_swap, self.zero)])
        self.sponge = [(b.s_out + t, r) for t in range(12)]
        self.inbuf, self.outbuf = [], self.sponge[:8]
        self.rows.append(r)

    def observe(self, source):
        self.outbuf = []
        self.inbuf.append(source)
        if len(self.inbuf) == 8:
            self._duplex()

    def get(self):
        if self.inbuf or not self.outbuf:
            self._duplex()
        return self.outbuf.pop()


class CircuitProver:
    """A circuit through the library's CircuitData (sipp_circuit_build / _prove / _verify): the constants_sigmas commitment and the schedule
    go to the device once; prove(inputs) generates the witness there and returns the flat proof."""

    def __init__(self, ctx, circ, fri=None, params=None, digest=None, zero_knowledge=False, seed=None, hasher="poseidon"):
        """hasher: "poseidon" (default: the circuit data as it always was) or "keccak" -- every Merkle tree of the commitment and of the
        proofs hashed with Keccak-256 truncated to 25 bytes (plonky2's KeccakGoldilocksConfig; the challenger stays Poseidon); it combines
        with zero_knowledge and with lookups.  ValueError for anything else.
        zero_knowledge: prove under fri.hiding = 1 -- salted oracles, and the circuit's blinding rows filled from `seed` (four canonical
        words; None: drawn from `secrets`), proof k under the seed with counter k.  ValueError if the FRI parameters need more blinding
        rows than the circuit carries (CircuitBuilder.declare_blinding)."""
        from . import _lib
        self.circ = c = circ
        if hasher not in _lib.HASHERS:
            raise ValueError("hasher must be 'poseidon' or 'keccak', not %r" % (hasher,))
        self.hasher = hasher
        self.params = params if params is not None else _lib.PlonkParams(c.num_routed, 8, 2)
        self.fri = fri if fri is not None else fri_params(c.log_n)
        if zero_knowledge:
            need, have = blinding_counts(self.fri, c.log_n), getattr(c, "blinding", (0, 0))
            if need[0] > have[0] or need[1] > have[1]:
                raise ValueError("zero knowledge: these FRI parameters need %d + 2 * %d blinding rows, the circuit carries %d + 2 * %d" % (need + have))
            hiding = _lib.FriParams.from_buffer_copy(self.fri)
            hiding.hiding = 1
            self.fri = hiding
        self.circuit = c.circuit()
        self._pc = _lib.PlonkCircuit.from_dict(self.circuit)
        self.data = _lib.CircuitData(ctx, c.log_n, self.params, self.fri, self._pc, c.constants_sigmas(), c.generators(), sched=c.schedule(),
                                     digest=digest, hasher=None if hasher == "poseidon" else hasher)
        if "lookup" in self.circuit:      # the description rides in circuit(): the multiplicities and the argument on every prove path
            self.data.set_lookup(self.circuit["lookup"])
        if zero_knowledge:
            import secrets
            self.data.set_blinding([secrets.randbelow(P) for _ in range(4)] if seed is None else seed)
        self.cap, self.digest = self.data.cap, self.data.digest

    def prove(self, *inputs):
        """inputs: the circuit's partial_witness arguments, the public_inputs arguments first"""
        c = self.circ
        return self.data.prove(c.partial_witness(*inputs), c.public_inputs(*inputs[:c.n_public_args]))

    def verify(self, proof):
        """-> (status, refusing stage): (0, 0) = accepted"""
        return self.data.verify(proof)

    def close(self):
        self.data.close()
