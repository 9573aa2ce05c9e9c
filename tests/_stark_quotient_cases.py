"""tests/_stark_quotient_cases.py -- crafted cells and challenges for the STARK prover's Z and quotient stages (no device).

sipp_k_z_columns and sipp_k_quotient (sipp_amd/csrc/prover.hip) are reached by the product only through whole proofs: every cell they
read is the LDE of an honest trace -- in effect a uniform field element -- and every challenge is what Fiat-Shamir hands out.  Their
kernels are written against BOUNDS on those inputs (canonical cells, a 1024-term lazy accumulator, the carry of a two-half limb
product), and uniform inputs meet such a bound with probability around 2^-32 per operation: the point tests/test_gpu_field_edges.py and
tests/_witness_edges.py make for the field headers and the witness generators.  This catalogue is their counterpart for the STARK side:

  cells       four styles of the tables lde [W][m], zlde [2 nc][m], aux [n_aux][m] (m = 2 N points of the quotient coset, leaf order):
              every cell p - 1, every cell 0, the value lattice laid out by a formula in (column class, column, natural index), uniform
              random; `carry`: random cells with every gadget's quotient limbs SOLVED so that the kernel's q * p limb product carries
              out of its low word (craft_q below); and `fold` (with alpha = (p - 1, p - 1), at log_n = 15 only): the lattice with the
              permuted inputs 0, the permuted tables 1 and Z 0, so that RestAcc F sums 1134 terms of hi32 = 2^32 - 1 times the middle limb
              of p - 1 and passes 2^64 unless it folds (rest_f_peak below)
  challenges  one random triple per case; the lattice in each of alpha, beta, gamma in turn (alpha = 0 in either component is REFUSED);
              beta = gamma (what lookup_rule = 1 produces)
  shapes      every entry of AIR_AIRS at the smallest trace its rows allow (both routes of quotient_rest), g2_u16 once at log_n = 15
              (the unsplit route with 378 checked columns: RestAcc folds, and in the `fold` case it has to)
  Z           synthetic one / two column layouts at log_n = 10, 13, 14, 20 (z_phase_a<4> in one and several blocks, <8>, and more than
              256 blocks: z_phase_b's chunk loops) and g1_u8's layout; the four styles, lattice challenges, vanishing numerators and
              vanishing DENOMINATORS at row 0, the last row, lane and block boundaries and twice in a column

Three readings take these cells: orc_eval_base (oracle/air.c, through orc_quotient_points), eval_constraints (oracle/py/stark_verify.py,
Python integers over the extension, fed the base point) and the device.  tests/test_oracle_stark_quotient_cases.py holds the first two
against each other and asserts reached(); tests/test_gpu_stark_quotient_cases.py holds the device against both.

The reference of Z is z_reference: Z[0] = 1, Z[r + 1] = Z[r] num[r] inv0(den[r]) in Python integers, inv0(0) = 0 -- the rule
oracle/plonk.c and plonk.hip follow for the wire permutation: a vanishing denominator stays out of any batch trick.
"""
import collections
import functools

import numpy as np

from oracle.py import plonky2_generic as g
from oracle.py import stark_verify as sv
from tests import _oracle
from tests import _witness_edges

P = 2 ** 64 - 2 ** 32 + 1
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
LATTICE = _witness_edges.MORE        # _gate_edges.EDGE_VALUES + (p - 2, 2^63, 2^32 + 1)
NL = len(LATTICE)
LAT_U64 = np.array(LATTICE, dtype=np.uint64)
GEN = 7
STYLES = ("pm1", "zero", "lattice", "random", "carry")
TABLE, UNCHECKED, CHECKED, PERM_IN, PERM_TAB, ZCOL, AUX = range(7)     # column classes

AIRS = sv.air_tables()[2]            # AIR_AIRS (data/air_tables.h), in its order: the probe selects by this index
P_LIMBS = sv.air_tables()[1]


def family(a):
    return {0: "curve", 1: "curve", 2: "fq12", 3: "mapg2", 6: "pairing"}[a["kind"]] + ("_hardened" if a["hardened"] else "")


FAMILIES = ("curve", "curve_hardened", "fq12", "mapg2", "pairing")


def bitrev(log_m):
    """rev[j] = the natural index of leaf position j (and back: the permutation is an involution)"""
    j = np.arange(1 << log_m, dtype=np.uint32)
    r = np.zeros_like(j)
    for b in range(log_m):
        r |= ((j >> b) & 1) << (log_m - 1 - b)
    return r


# ---------------------------------------------------------------------------------------------------- the lattice formula
def lattice_index(cls, c, i):
    """index into LATTICE of the cell of column c (class cls) at natural index i.  Only + * >> & %, on non-negative int64: numpy arrays
    and torch tensors both take it (the log_n = 15 tables are built on the device from the same formula).  For a fixed column and
    i = 16 k + r the index moves by 17 k = 8 k (mod 9): every column holds every lattice value, and since every point is the `local` row
    of itself and the `next` row of the point two natural indices before it, every class sees every value in both roles."""
    return (c * (1 + (i & 7)) + 4 * cls + i + (i >> 4)) % NL


def lde_classes(a):
    nm, nc, cb = a["n_main"], a["n_checked"], a["checked_base"]
    cls = np.empty(nm + 2 * nc, dtype=np.int64)
    cls[0], cls[1:cb], cls[cb:nm], cls[nm:nm + nc], cls[nm + nc:] = TABLE, UNCHECKED, CHECKED, PERM_IN, PERM_TAB
    return cls


def lattice_cells(cls, cols, nat):
    """[len(cols)][len(nat)] uint64"""
    idx = lattice_index(np.asarray(cls, dtype=np.int64)[:, None], np.asarray(cols, dtype=np.int64)[:, None], np.asarray(nat, dtype=np.int64)[None, :])
    return LAT_U64[idx]


def class_tables(a, style, nat):
    """(lde [W][len(nat)], zlde [2 nc][len(nat)], aux [n_aux][len(nat)]) of the styles that are a formula in (column class, column, natural
    index), at the natural indices nat: pm1, zero, lattice, and fold -- the lattice, but every permuted input 0, every permuted table 1 and
    every Z cell 0, so that pin - ptab = Z - 1 = p - 1 in every checked column at every point"""
    W, nz, na = a["n_main"] + 2 * a["n_checked"], 2 * a["n_checked"], a["n_aux"]
    if style in ("pm1", "zero"):
        return tuple(np.full((c, len(nat)), P - 1 if style == "pm1" else 0, dtype=np.uint64) for c in (W, nz, na))
    assert style in ("lattice", "fold")
    cls = lde_classes(a)
    lde, zlde, aux = (lattice_cells(cls, np.arange(W), nat), lattice_cells(np.full(nz, ZCOL), np.arange(nz), nat),
                      lattice_cells(np.full(na, AUX), np.arange(na), nat))
    if style == "fold":
        lde[cls == PERM_IN], lde[cls == PERM_TAB], zlde[:] = 0, 1, 0
    return lde, zlde, aux


# ---------------------------------------------------------------------------------------------------- gadgets and the q * p carry
Gadget = collections.namedtuple("Gadget", "sign_col q_terms n_products")


@functools.lru_cache(maxsize=None)
def gadgets(ai):
    """the gadgets of AIRS[ai]: sign column, the terms (coef, base, stride) of the 17-limb quotient vector, the number of products"""
    prog, pos, out = AIRS[ai]["prog"], 0, []

    def skip_vec():
        nonlocal pos
        pos += 2 + 5 * prog[pos + 1]
    while pos < len(prog) and prog[pos] == 1:
        sign_col = prog[pos + 1]
        pos += 7
        assert prog[pos] == 17
        terms = [tuple(prog[pos + 2 + 5 * t: pos + 7 + 5 * t]) for t in range(prog[pos + 1])]
        assert all(t[3] < 0 for t in terms), "a flagged quotient vector: the crafted limbs would depend on the point"
        skip_vec()
        n_products = prog[pos]
        pos += 1
        for _ in range(n_products):
            pos += 1
            skip_vec()
            skip_vec()
        n_linear = prog[pos]
        pos += 1
        for _ in range(n_linear):
            pos += 1
            skip_vec()
        out.append(Gadget(sign_col, tuple(t[:3] for t in terms), n_products))
    return tuple(out), pos


@functools.lru_cache(maxsize=None)
def poly_coefficients(ai):
    """how many monomials of the polynomial constraints of AIRS[ai] have coefficient +1, -1, anything else (the three paths of the
    lazy POLY fold: gl::add, gl::sub, gl::mad)"""
    prog = AIRS[ai]["prog"]
    pos = gadgets(ai)[1]
    cnt = {"+1": 0, "-1": 0, "other": 0}
    while pos < len(prog):
        nmono = prog[pos + 1]
        pos += 2
        for _ in range(nmono):
            coef, nf = prog[pos], prog[pos + 1]
            pos += 2 + 2 * nf
            cnt["+1" if coef == 1 else "-1" if coef == -1 else "other"] += 1
    return cnt


def qp_carries(q):
    """the output coefficients k at which the kernel's q * p limb product carries: its model in integers --
    al = sum lo32(q_i) p_(k-i), ah = sum hi32(q_i) p_(k-i), l = al + (ah << 32) mod 2^64, carry iff l < al"""
    fired = []
    for k in range(32):
        al = sum((q[i] & M32) * P_LIMBS[k - i] for i in range(17) if 0 <= k - i < 16)
        ah = sum((q[i] >> 32) * P_LIMBS[k - i] for i in range(17) if 0 <= k - i < 16)
        assert al < 1 << 64 and ah < 1 << 64
        if (al + (ah << 32)) & M64 < al:
            fired.append(k)
    return fired


def craft_q(ai, gi):
    """17 canonical quotient limbs of gadget gi that fire the carry at output coefficient k = (3 gi + kind) mod 17: the limbs below k
    from the lattice and a fixed seed, lo32(q_k) all ones (so al >= 2^33), hi32(q_k) SOLVED modulo 2^32 so that lo32(ah) is all ones --
    p's low limb is odd -- and then al + (ah << 32) passes 2^64.  A deterministic search in the manner of _witness_edges.crafted_state."""
    k = (3 * gi + AIRS[ai]["kind"]) % 17
    rng = np.random.default_rng(7000 + 100 * ai + gi)
    p0_inv = pow(P_LIMBS[0], -1, 1 << 32)
    while True:
        q = [int(x) for x in rng.integers(0, P, size=17, dtype=np.uint64)]
        for i in range(0, k, 3):
            q[i] = LATTICE[int(rng.integers(0, NL))]
        rest = sum((q[i] >> 32) * P_LIMBS[k - i] for i in range(k) if k - i < 16)
        for target in (M32, M32 - 1):
            hi = (target - rest) * p0_inv & M32
            q[k] = hi << 32 | M32
            if q[k] < P and k in qp_carries(q):
                return q, k


def q_cells(ai):
    """{column: value} for the `carry` style: every gadget's quotient limbs crafted; a limb of several cells (the u8 tables: lo + 256 hi)
    takes its value in the coefficient-1 cell and zero in the others"""
    cells = {}
    for gi, gd in enumerate(gadgets(ai)[0]):
        q, _ = craft_q(ai, gi)
        assert gd.q_terms[0][0] == 1
        for t, (coef, base, stride) in enumerate(gd.q_terms):
            for i in range(17):
                cells[base + i * stride] = q[i] if t == 0 else 0
    return cells


def q_of_cells(ai, gi, cell):
    """the quotient vector the kernel's qvec<17> computes from the cells of one point (cell: column -> value)"""
    return [sum(coef * cell(base + i * stride) for coef, base, stride in gadgets(ai)[0][gi].q_terms) % P for i in range(17)]


# ---------------------------------------------------------------------------------------------------- quotient cases
QCase = collections.namedtuple("QCase", "name ai log_n style alpha beta gamma seed")


def _rand_pair(rng):
    return tuple(int(x) for x in rng.integers(1, P, size=2, dtype=np.uint64))


def small_log_n(a):
    return max(10, a["log_rows"])


@functools.lru_cache(maxsize=None)
def quotient_cases():
    out = []

    def add(tag, ai, log_n, style, alpha=None, beta=None, gamma=None):
        seed = 100 * len(out) + 17
        rng = np.random.default_rng(seed)
        r = [_rand_pair(rng) for _ in range(3)]
        out.append(QCase("%s@%d-%s%s" % (AIRS[ai]["name"], log_n, style, tag), ai, log_n, style, alpha or r[0], beta or r[1], gamma or r[2], seed))
    for ai, a in enumerate(AIRS):                       # every AIR, every style, a random triple
        for style in STYLES:
            add("", ai, small_log_n(a), style)
    for which in ("alpha", "beta", "gamma"):             # the lattice in each challenge in turn, both components (g1_u16, lattice cells)
        for k in range(NL):
            add("-%s=L%d" % (which, k), 0, 10, "lattice", **{which: (LATTICE[k], LATTICE[(k + 4) % NL])})
    for fam in FAMILIES:                                 # beta = gamma: lookup_rule's shared challenge
        ai = next(i for i, a in enumerate(AIRS) if family(a) == fam)
        bg = _rand_pair(np.random.default_rng(900 + ai))
        add("-beta=gamma", ai, small_log_n(AIRS[ai]), "lattice", beta=bg, gamma=bg)
    return tuple(out)


BIG_AI = 1                                               # g2_u16 at log_n = 15: unsplit, 378 checked columns


@functools.lru_cache(maxsize=None)
def big_cases():
    assert AIRS[BIG_AI]["name"] == "g2_u16"
    out = []
    for n, style in enumerate(("pm1", "lattice", "fold")):
        rng = np.random.default_rng(5000 + n)
        r = [_rand_pair(rng) for _ in range(3)]
        # fold: alpha = p - 1 has order 2 and every weight of F's column terms is an ODD power of it (rest_f_peak), p - 1 itself
        out.append(QCase("g2_u16@15-%s" % style, BIG_AI, 15, style, (P - 1, P - 1) if style == "fold" else r[0], r[1], r[2], 5000 + n))
    return tuple(out)


def big_gather(case, pos):
    """the cells the references need of a table too large for the host: (need, slot, (lde, zlde, aux)) -- the leaf positions pos and those
    of their next rows, where each lies in the gathered tables, and the tables [.][len(need)] from the catalogue's formula"""
    log_m = case.log_n + 1
    m, rev = 1 << log_m, bitrev(log_m)
    pos = np.asarray(pos, dtype=np.int64)
    need = np.unique(np.concatenate([pos, rev[(rev[pos].astype(np.int64) + 2) & (m - 1)]])).astype(np.int64)
    slot = np.zeros(m, dtype=np.uint32)
    slot[need] = np.arange(len(need), dtype=np.uint32)
    return need, slot, class_tables(AIRS[case.ai], case.style, rev[need])


def refused(case):
    return 0 in case.alpha


def tables(case):
    """(lde [W][m], zlde [2 nc][m], aux [n_aux][m]) uint64, leaf order, every cell canonical"""
    a = AIRS[case.ai]
    m = 2 << case.log_n
    W, nz, na = a["n_main"] + 2 * a["n_checked"], 2 * a["n_checked"], a["n_aux"]
    shapes = ((W, m), (nz, m), (na, m))
    if case.style in ("pm1", "zero", "lattice", "fold"):
        return class_tables(a, case.style, bitrev(case.log_n + 1))
    rng = np.random.default_rng(case.seed + 1)
    tabs = tuple(np.ascontiguousarray(rng.integers(0, P, size=s, dtype=np.uint64)) for s in shapes)
    if case.style == "carry":
        for col, v in q_cells(case.ai).items():
            tabs[0][col, :] = v
    return tabs


def sample_positions(log_n, seed=1):
    """8 leaf positions: natural indices 0 and 1 (both parities), m - 2 and m - 1 (their `next` row wraps to 0 and 1), m / 2 and
    m / 2 + 1, two more from a fixed seed"""
    m = 2 << log_n
    nat = [0, 1, m - 2, m - 1, m // 2, m // 2 + 1] + [int(x) for x in np.random.default_rng(seed).integers(2, m - 2, size=2)]
    rev = bitrev(log_n + 1)
    return np.array([rev[i] for i in nat], dtype=np.uint32)


def big_sample(log_n=15):
    """4096 leaf positions: the first and last 64, the first and last point of every 256-point block, the rest from a fixed seed"""
    m = 2 << log_n
    fixed = set(range(64)) | set(range(m - 64, m)) | set(range(0, m, 256)) | set(range(255, m, 256))
    rng = np.random.default_rng(15)
    while len(fixed) < 4096:
        fixed.add(int(rng.integers(0, m)))
    return np.array(sorted(fixed), dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------- the Python reading at a base point
@functools.lru_cache(maxsize=None)
def _vper_coeffs(ai):
    a = AIRS[ai]
    cache, out = {}, []
    for k in range(a["n_vflag"] + a["n_vconst"]):
        vals = tuple(v % P for v in sv.vper_values(a, k))
        if vals not in cache:
            cache[vals] = g.ifft(list(vals))
        out.append(cache[vals])
    return out


@functools.lru_cache(maxsize=None)
def point_values(ai, log_n, i):
    """at the point x = 7 w_2N^i, in Python integers: (periodic and value-periodic values, lag_first, lag_last, z_last, 1 / Z_H(x))"""
    a = AIRS[ai]
    n = 1 << log_n
    x = GEN * pow(g.primitive_root_of_unity(log_n + 1), i, P) % P
    per = [sv.periodic_at(log_n, mk, r0, g.Ext(x)) for mk, r0 in sv.air_tables()[0]]
    assert all(v[1] == 0 for v in per)
    y = pow(x, 1 << (log_n - a["log_rows"]), P)
    memo = {}
    for co in _vper_coeffs(ai):
        if id(co) not in memo:
            acc = 0
            for c in reversed(co):
                acc = (acc * y + c) % P
            memo[id(co)] = g.Ext(acc)
        per.append(memo[id(co)])
    gi = g.inv(g.primitive_root_of_unity(log_n))
    zh = (pow(x, n, P) - 1) % P
    ninv = g.inv(n)
    lag_first = zh * ninv * g.inv((x - 1) % P) % P
    lag_last = zh * ninv * gi * g.inv((x - gi) % P) % P
    return per, lag_first, lag_last, (x - gi) % P, g.inv(zh)


def python_quotient(case, cell, zcell, auxcell, j):
    """eval_constraints (oracle/py/stark_verify.py) at the base point of leaf position j, embedded in the extension, times 1 / Z_H:
    the two quotient values as integers.  cell(c, pos) / zcell / auxcell read one cell at a leaf position."""
    a = AIRS[case.ai]
    log_m = case.log_n + 1
    m = 1 << log_m
    rev = bitrev(log_m)
    i = int(rev[j])
    jn = int(rev[(i + 2) & (m - 1)])
    W, nz = a["n_main"] + 2 * a["n_checked"], 2 * a["n_checked"]
    E = g.Ext
    per, lf, ll, zl, zh_inv = point_values(case.ai, case.log_n, i)
    acc = sv.eval_constraints(a, case.log_n, [E(cell(c, j)) for c in range(W)], [E(cell(c, jn)) for c in range(W)],
                              [E(auxcell(c, j)) for c in range(a["n_aux"])], per, [E(zcell(c, j)) for c in range(nz)],
                              [E(zcell(c, jn)) for c in range(nz)], E(lf), E(ll), E(zl), case.alpha, case.beta, case.gamma)
    assert acc[0][1] == 0 and acc[1][1] == 0, "a base point left the base field"
    return [acc[0][0] * zh_inv % P, acc[1][0] * zh_inv % P]


def check_two_readings(case, lde, zlde, aux, pos, slot=None):
    """orc_eval_base against eval_constraints at the leaf positions pos; returns the oracle's values [2][len(pos)]"""
    ref = _oracle.quotient_points(case.ai, case.log_n, lde, zlde, aux, case.alpha, case.beta, case.gamma, pos, slot)
    at = (lambda j: int(slot[j])) if slot is not None else (lambda j: j)
    for q, j in enumerate(pos):
        py = python_quotient(case, lambda c, p: int(lde[c, at(p)]), lambda c, p: int(zlde[c, at(p)]), lambda c, p: int(aux[c, at(p)]), int(j))
        assert [int(ref[0, q]), int(ref[1, q])] == py, "%s: orc_eval_base and eval_constraints differ at leaf position %d" % (case.name, j)
    return ref


# ---------------------------------------------------------------------------------------------------- Z cases
ZCase = collections.namedtuple("ZCase", "name log_n n_main cbase nc style beta gamma seed patches")
G1_U8 = next(i for i, a in enumerate(AIRS) if a["name"] == "g1_u8")


def z_rows(log_n):
    return 8 if (1 << log_n) >= 16384 else 4       # rows per lane (sipp_k_z_columns)


def z_blocks(log_n):
    return (1 << log_n) // (256 * z_rows(log_n))


@functools.lru_cache(maxsize=None)
def z_cases():
    out = []

    def add(tag, log_n, layout, style, beta=None, gamma=None, patches=()):
        seed = 31 * len(out) + 5
        rng = np.random.default_rng(seed)
        r = [_rand_pair(rng) for _ in range(2)]
        out.append(ZCase("z@%d-nc%d-%s%s" % (log_n, layout[2], style, tag), log_n, layout[0], layout[1], layout[2], style, beta or r[0],
                         gamma or r[1], seed, tuple(patches)))
    two, one = (3, 1, 2), (2, 1, 1)                   # (n_main, checked_base, n_checked): table | checked | permuted in | permuted table
    real = (AIRS[G1_U8]["n_main"], AIRS[G1_U8]["checked_base"], AIRS[G1_U8]["n_checked"])
    for log_n in (10, 13, 14):
        for style in ("pm1", "zero", "lattice", "random"):
            add("", log_n, two, style)
    for style in ("lattice", "random"):
        add("", 10, real, style)
        add("", 20, one, style)
    for which in ("beta", "gamma"):                    # the lattice in each challenge (with gamma = 0 on zero cells EVERY denominator vanishes)
        for k in range(NL):
            for style in ("lattice", "zero"):
                add("-%s=L%d" % (which, k), 10, two, style, **{which: (LATTICE[k], LATTICE[(k + 4) % NL])})
    for log_n in (10, 13, 14):
        n, zr = 1 << log_n, z_rows(log_n)
        last_block = (z_blocks(log_n) - 1) * 256 * zr
        # a numerator that vanishes: col + gamma_0 = 0, tab + beta_1 = 0
        add("-num=0", log_n, two, "random", patches=[("col", 0, 0, 5), ("tab", 0, 1, n - 3)])
        spots = {"row0": [0], "last": [n - 1], "lane": [zr * 3], "lane-1": [zr * 3 - 1], "block": [last_block], "block-1": [max(last_block, 256 * zr) - 1],
                 "twice": [zr * 7 + 1, n // 2 + 3]}
        for tag, rows in spots.items():
            # pin + gamma = 0 in column 0 under challenge 0, ptab + beta = 0 in column 1 under challenge 1: the other (column, challenge)
            # pairs of the same cells stay regular, and so do their Z columns
            add("-den=0@%s" % tag, log_n, two, "random", patches=[("pin", 0, 0, r) for r in rows] + [("ptab", 1, 1, r) for r in rows])
    add("-den=0@row0", 10, real, "random", patches=[("pin", 5, 0, 0), ("ptab", 377, 1, 0)])
    return tuple(out)


def z_trace(case):
    """[n_main + 2 nc][N] uint64, natural row order"""
    nm, nc, cb, n = case.n_main, case.nc, case.cbase, 1 << case.log_n
    W = nm + 2 * nc
    if case.style in ("pm1", "zero"):
        t = np.full((W, n), P - 1 if case.style == "pm1" else 0, dtype=np.uint64)
    elif case.style == "lattice":
        t = lattice_cells(lde_classes(dict(n_main=nm, n_checked=nc, checked_base=cb)), np.arange(W), np.arange(n))
    else:
        t = np.ascontiguousarray(np.random.default_rng(case.seed + 1).integers(0, P, size=(W, n), dtype=np.uint64))
    for what, j, i, r in case.patches:
        col, ch = {"col": (cb + j, case.gamma), "tab": (0, case.beta), "pin": (nm + j, case.gamma), "ptab": (nm + nc + j, case.beta)}[what]
        t[col, r] = (P - ch[i]) % P
    return t


def z_num_den(case, trace, zi):
    """numerators and denominators of Z column zi = i nc + j, as lists of Python integers"""
    i, j = divmod(zi, case.nc)
    b, gm = case.beta[i], case.gamma[i]
    col, tab, pin, ptab = (trace[c].tolist() for c in (case.cbase + j, 0, case.n_main + j, case.n_main + case.nc + j))
    num = [(c + gm) * (t + b) % P for c, t in zip(col, tab)]
    den = [(p + gm) * (q + b) % P for p, q in zip(pin, ptab)]
    return num, den


def z_reference(case, trace):
    """[2 nc][N] uint64: Z[0] = 1, Z[r + 1] = Z[r] num[r] inv0(den[r]), cell by cell in Python integers; inv0(0) = 0"""
    n = 1 << case.log_n
    out = np.empty((2 * case.nc, n), dtype=np.uint64)
    for zi in range(2 * case.nc):
        num, den = z_num_den(case, trace, zi)
        z, col = 1, []
        for r in range(n):
            col.append(z)
            z = z * num[r] * (pow(den[r], -1, P) if den[r] else 0) % P
        out[zi] = col
    return out


def z_relation_holds(case, trace, zv):
    """Z[0] = 1 and Z[r + 1] den[r] == Z[r] num[r] on every row r < N - 1, in exact integers (object arrays): pins Z when no denominator
    vanishes (asserted)"""
    for zi in range(2 * case.nc):
        i, j = divmod(zi, case.nc)
        o = lambda c: trace[c].astype(object)
        num = (o(case.cbase + j) + case.gamma[i]) * (o(0) + case.beta[i]) % P
        den = (o(case.n_main + j) + case.gamma[i]) * (o(case.n_main + case.nc + j) + case.beta[i]) % P
        assert (den != 0).all(), "the relation pins Z only where no denominator vanishes"
        z = zv[zi].astype(object)
        if int(z[0]) != 1 or not ((z[1:] * den[:-1] - z[:-1] * num[:-1]) % P == 0).all():
            return False
    return True


# ---------------------------------------------------------------------------------------------------- reach
def rest_chunks(log_n, nc):
    """sipp_quotient_rest_chunks (sipp_amd/csrc/prover.hpp), restated: ranges of checked columns on a thin domain; 1 = the unsplit route"""
    if log_n + 1 > 15:
        return 1
    c = min(nc // 32, 16)
    return c if c > 1 else 1


def rest_folds(log_n, nc):
    """how often RestAcc F (three terms per checked column, counted two columns at a time, folded at 960) folds in one lane"""
    chunks = rest_chunks(log_n, nc)
    per = nc if chunks == 1 else ((nc + chunks - 1) // chunks + 1) // 2 * 2
    terms = folds = 0
    for _ in range(0, per, 2):
        terms += 6
        if terms >= 960:
            folds, terms = folds + 1, 0
    return folds


def limbs3(c):
    """gl::limbs3: c = l0 + l1 2^22 + l2 2^44"""
    return c & 0x3FFFFF, (c >> 22) & 0x3FFFFF, c >> 44


def rest_f_peak(case, lde, zlde, fold_at=960):
    """the largest value any of the six sums of RestAcc F takes, for either challenge, on the unsplit walk of quotient_rest_kernel over the
    cells of ONE point (lde [W], zlde [2 nc]: its local row), in integers: F's model.  Its terms are the range table's first-row
    constraint (not counted) and, per checked column k, pin - ptab, Z_0 - 1 and Z_1 - 1 under the weights alpha_c^e with
    e = K - 1 - (3 + 2 k) - {0, 2 nc, 4 nc}, K = 3 + 6 nc (alpha_pow3_kernel, slots 0, 2, 4); a term adds lo32(v) l_q to sum q and
    hi32(v) l_q to sum 3 + q, l = limbs3 of the weight; the terms are counted six per pair of columns and the sums are emptied when the
    count reaches fold_at (None: never).  A sum that passes 2^64 wraps on the device."""
    a = AIRS[case.ai]
    nm, nc = a["n_main"], a["n_checked"]
    assert rest_chunks(case.log_n, nc) == 1
    K, peak = 3 + 6 * nc, 0
    for c in range(2):
        acc, terms = [0] * 6, 0

        def mac(v, e):
            w = limbs3(pow(case.alpha[c], e, P))
            for q in range(3):
                acc[q] += (v & M32) * w[q]
                acc[3 + q] += (v >> 32) * w[q]
            return max(acc)
        peak = max(peak, mac(int(lde[0]), K - 1))
        for k0 in range(0, nc, 2):
            for k in range(k0, min(k0 + 2, nc)):
                e = K - 1 - (3 + 2 * k)
                for v, ex in (((int(lde[nm + k]) - int(lde[nm + nc + k])) % P, e), ((int(zlde[k]) - 1) % P, e - 2 * nc),
                              ((int(zlde[nc + k]) - 1) % P, e - 4 * nc)):
                    peak = max(peak, mac(v, ex))
            terms += 6
            if fold_at is not None and terms >= fold_at:
                acc, terms = [0] * 6, 0
    return peak


def reached():
    """what the catalogue reaches, written from the programs and the shapes (the CPU test asserts every item)"""
    r = dict(route={}, fold={}, fold_needed={}, sliced={}, carry={}, odd_clamp={}, poly_coefficients={}, z_rows={}, z_blocks={}, z_chunk_loop={})
    for case in big_cases():
        # (the peak of F's sums at the point of leaf position 0 as the kernel folds, the same with no fold): the fold is NEEDED where the
        # second passes 2^64 (the cells of a class-formula style at one natural index)
        lde, zlde, _ = class_tables(AIRS[case.ai], case.style, bitrev(case.log_n + 1)[:1])
        r["fold_needed"][case.name] = (rest_f_peak(case, lde[:, 0], zlde[:, 0]), rest_f_peak(case, lde[:, 0], zlde[:, 0], fold_at=None))
    for case in quotient_cases() + big_cases():
        a = AIRS[case.ai]
        chunks = rest_chunks(case.log_n, a["n_checked"])
        r["route"][case.name] = "split" if chunks > 1 else "unsplit"
        r["fold"][case.name] = rest_folds(case.log_n, a["n_checked"]) > 0
        r["sliced"][case.name] = any(gd.n_products > 64 for gd in gadgets(case.ai)[0])
        # a range of the split route (or the whole unsplit walk) with an odd number of columns: the second slot of its last pair is
        # clamped to column nc - 1 and masked out
        per = a["n_checked"] if chunks == 1 else ((a["n_checked"] + chunks - 1) // chunks + 1) // 2 * 2
        r["odd_clamp"][case.name] = any((min(a["n_checked"], k + per) - k) % 2 for k in range(0, a["n_checked"], per))
        if case.style == "carry":
            cells = q_cells(case.ai)
            r["carry"][case.name] = [(gi, k) for gi in range(len(gadgets(case.ai)[0])) for k in qp_carries(q_of_cells(case.ai, gi, cells.__getitem__))]
    for ai, a in enumerate(AIRS):
        r["poly_coefficients"][a["name"]] = poly_coefficients(ai)
    for case in z_cases():
        r["z_rows"][case.name] = z_rows(case.log_n)
        r["z_blocks"][case.name] = z_blocks(case.log_n)
        r["z_chunk_loop"][case.name] = z_blocks(case.log_n) > 256
    return r
