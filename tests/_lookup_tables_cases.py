"""Several tagged lookup tables and the lookup generator, read in exact Python integers (include/sipp_hip.h "LOOKUP TABLES", description
word 7 = tag_const0, and SIPP_GEN_LOOKUP): a catalogue of explicit instances and the reading of the multiplicities, the running-sum
columns S / U, the argument's terms on a row and the verifier's equation at zeta, all with the tag term eta^2 tag(row) in every
combination; then the generator's rule  y = table[x]  for a dense table, with its instances.  The untagged reading is
tests/_lookup_cases.py, whose helpers this file uses where the tag does not enter.  CPU only.  Used by
tests/test_lookup_tables_reading.py, tests/test_lookup_tables_builder.py and tests/test_gpu_lookup_tables.py.

An entry is a dict like tests/_lookup_cases.py's, with desc[7] != 0, `tables`: [(the looking rows' tag word, the table rows' tag word, table rows,
looking rows)] and `entries`: every table's distinct pairs."""
import functools

import numpy as np

from tests import _lookup_cases as lc

P = lc.P
E_BADARG, E_WITNESS = lc.E_BADARG, lc.E_WITNESS
Absent, Vanishing = lc.Absent, lc.Vanishing
first_mismatch, group_slots = lc.first_mismatch, lc.group_slots


def unpack(desc):
    return tuple(int(x) for x in desc)


def row_tags(desc, consts, i):
    """(the looking tag, the table tag) of row i as field values; (0, 0) without tag columns"""
    t0 = int(desc[7])
    return (int(consts[t0][i]) % P, int(consts[t0 + 1][i]) % P) if t0 else (0, 0)


# ---- the reading -----------------------------------------------------------------------------------------------------------------------
def multiplicities(desc, wires, consts):
    """lc.multiplicities with the entry (tag, x, y): the table row's tag against the looking row's.  Raises Absent."""
    q_look, lw, n_look, q_tab, tc, tm, n_tab, _ = unpack(desc)
    out = np.array(wires, dtype=np.uint64).copy()
    n = out.shape[1]
    first = {}
    for i in range(n):
        if int(consts[q_tab][i]) % P:
            tag = row_tags(desc, consts, i)[1]
            for k in range(n_tab):
                out[tm + k][i] = 0
                first.setdefault((tag, int(consts[tc + 2 * k][i]) % P, int(consts[tc + 2 * k + 1][i]) % P), (tm + k, i))
    counts = {}
    for i in range(n):
        if int(consts[q_look][i]) % P:
            tag = row_tags(desc, consts, i)[0]
            for k in range(n_look):
                key = (tag, int(out[lw + 2 * k][i]) % P, int(out[lw + 2 * k + 1][i]) % P)
                if key not in first:
                    raise Absent((i, k, key))
                counts[first[key]] = counts.get(first[key], 0) + 1
    for (col, i), v in counts.items():
        out[col][i] = v
    return out


def denominators(desc, wires, consts, i, looking, slots, eta, theta):
    """the d_k = theta - (x_k + eta y_k + eta^2 tag_look(i)) or (e_k, m_k) of a group on row i: the untagged reading under
    theta - eta^2 tag, which is the same field element"""
    tag = row_tags(desc, consts, i)[0 if looking else 1]
    return lc.denominators(desc[:7] + (0,), wires, consts, i, looking, slots, eta, (theta - eta * eta * tag) % P)


def sums(desc, wires, consts, D, etas, thetas):
    """lc.sums with the tagged denominators: ([C J][N] uint64, closes).  Raises Vanishing."""
    q_look, q_tab = int(desc[0]), int(desc[3])
    n = np.asarray(wires).shape[1]
    gs = group_slots(desc, D)
    J = len(gs)
    s_cols, u_cols, closes = [], [], True
    for eta, theta in zip(etas, thetas):
        eta, theta = eta % P, theta % P
        s, us, acc = [], [[] for _ in range(J - 1)], 0
        for i in range(n):
            s.append(acc)
            for j, (looking, slots) in enumerate(gs):
                q = int(consts[q_look if looking else q_tab][i]) % P
                if q:
                    step = 0
                    for d, m in denominators(desc, wires, consts, i, looking, slots, eta, theta):
                        if d == 0:
                            raise Vanishing((i, j))
                        step += m * pow(d, -1, P)
                    acc = (acc + (q * step if looking else -q * step)) % P
                if j < J - 1:
                    us[j].append(acc)
        closes &= acc == 0
        s_cols.append(s)
        u_cols += us
    return np.array(s_cols + u_cols, dtype=np.uint64), closes


def terms_on_row(desc, wires, consts, D, cols, C, c, eta, theta, i):
    """lc.terms_on_row under the row's own theta - eta^2 tag, group by group (a looking and a table group of one row differ in tag)"""
    gs = group_slots(desc, D)
    eta, theta = eta % P, theta % P
    tl, tt = row_tags(desc, consts, i)
    as_l = lc.terms_on_row(desc[:7] + (0,), wires, consts, D, cols, C, c, eta, (theta - eta * eta * tl) % P, i)
    as_t = lc.terms_on_row(desc[:7] + (0,), wires, consts, D, cols, C, c, eta, (theta - eta * eta * tt) % P, i)
    return [as_l[0]] + [(as_l if looking else as_t)[1 + j] for j, (looking, _) in enumerate(gs)]


def all_terms_vanish(e, wires, cols):
    n = 1 << e["log_n"]
    return all(t == 0 for c in range(e["C"]) for i in range(n)
               for t in terms_on_row(e["desc"], wires, e["consts"], e["D"], cols, e["C"], c, e["etas"][c], e["thetas"][c], i))


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------
def build(name, log_n, D, C, n_look, n_tab, tables, seed, *, shared=0, classes=()):
    """Constants: column 0 the selector, q_look, q_tab, the 2 n_tab table columns, the two tag columns.  Wires: one filler, the 2 n_look
    looking wires, the n_tab multiplicity wires.  tables: [(tag word of its looking rows, tag word of its table rows, table rows,
    looking rows)] -- the two words are the same field value.  Every table has distinct random entries of its own; the first `shared`
    entries of table 0 are also the first entries of every other table (the same (x, y) under every tag), and every looking row's slot
    0 looks entry 0 up, so a shared pair is counted under each tag.  Unmarked rows hold garbage everywhere, the tag columns included."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    q_look, q_tab, tab_const0 = 1, 2, 3
    tag_const0 = tab_const0 + 2 * n_tab
    K, W = tag_const0 + 2, 1 + 2 * n_look + n_tab
    desc = (q_look, 1, n_look, q_tab, tab_const0, 1 + 2 * n_look, n_tab, tag_const0)
    consts, wires = lc._rand(rng, (K, n)), lc._rand(rng, (W, n))
    consts[0] = 0
    consts[q_look], consts[q_tab] = 0, 0
    seen, ents = set(), []
    for t, (tag_l, tag_t, trows, lrows) in enumerate(tables):
        assert tag_l % P == tag_t % P and not any(consts[q_tab][list(trows)]) and not any(consts[q_look][list(lrows)])
        consts[q_tab][list(trows)] = 1
        consts[q_look][list(lrows)] = 1
        consts[tag_const0][list(lrows)] = tag_l
        consts[tag_const0 + 1][list(trows)] = tag_t
        want = len(trows) * n_tab
        ent = list(ents[0][:shared]) if t else []
        while len(ent) < want:
            xy = (int(lc._rand(rng, ())) & 0xFFFF, int(lc._rand(rng, ())) & 0xFF)
            if xy not in seen:
                seen.add(xy)
                ent.append(xy)
        ents.append(ent)
        slots = (ent + [ent[-1]] * (len(trows) * n_tab))[:len(trows) * n_tab]
        for s, (x, y) in enumerate(slots):
            i, k = trows[s // n_tab], s % n_tab
            consts[tab_const0 + 2 * k][i], consts[tab_const0 + 2 * k + 1][i] = x, y
        for i in lrows:
            for k in range(n_look):
                x, y = ent[0] if k == 0 else ent[int(rng.integers(0, len(ent)))]
                wires[1 + 2 * k][i], wires[2 + 2 * k][i] = x, y
    etas, thetas = [int(v) for v in lc._rand(rng, (C,))], [int(v) for v in lc._rand(rng, (C,))]
    return dict(name=name, log_n=log_n, D=D, C=C, num_selectors=1, desc=desc, wires=wires, consts=consts, etas=etas, thetas=thetas,
                classes=set(classes), expect="ok", tables=[(a, b, list(c), list(d)) for a, b, c, d in tables], entries=ents,
                table_rows=sorted(r for t in tables for r in t[2]), look_rows=sorted(r for t in tables for r in t[3]))


def _entry(fn):
    return functools.lru_cache(maxsize=None)(fn)


@_entry
def n4_one_row_each():
    """N = 4: one table row under tag 0, one under tag 1, one looking row each"""
    return build("n4_one_row_each", 2, 2, 1, 1, 1, [(0, 0, [2], [0]), (1, 1, [3], [1])], 31, classes={"n4_single_rows"})


@_entry
def n8_D2_straddle_C8_shared():
    """N = 8, D = 2, n_look = n_tab = D + 1 (every row's slots straddle two groups), eight challenges; entry 0 is shared"""
    return build("n8_D2_straddle_C8_shared", 3, 2, 8, 3, 3, [(0, 0, [0, 5], [1, 2]), (1, 1, [6], [7, 3])], 32, shared=1,
                 classes={"groups_straddle", "eight_challenges", "same_pair_under_both_tags", "row0_marked"})


@_entry
def n16_big_tags_and_words_plus_p():
    """three tables: a tag of 2^63 + 5, a tag 7 whose looking rows say 7 and whose table rows say 7 + p, and tag 0 given as p; the
    first two entries are shared by all three"""
    return build("n16_big_tags_and_words_plus_p", 4, 2, 2, 2, 3, [((1 << 63) + 5, (1 << 63) + 5, [0, 1], [2, 3]), (7, 7 + P, [4], [5, 6, 7]),
                                                                  (P, 0, [8, 9], [15])], 33, shared=2,
                 classes={"tags_ge_2_63", "tag_words_plus_p", "same_pair_under_both_tags", "three_tables", "last_row_marked"})


@_entry
def n1024_D8_two_tables():
    """N = 1024, D = 8: several blocks, the two-level scan, groups that straddle; the whole proof's instance"""
    return build("n1024_D8_two_tables", 10, 8, 2, 9, 9, [(0, 0, list(range(0, 1024, 74)), list(range(5, 1024, 11))),
                                                         (1, 1, list(range(37, 1024, 74)), list(range(6, 1024, 11)))], 34, shared=5,
                 classes={"several_blocks", "groups_straddle", "same_pair_under_both_tags", "row0_marked"})


ENTRIES = [n4_one_row_each, n8_D2_straddle_C8_shared, n16_big_tags_and_words_plus_p, n1024_D8_two_tables]


def _spoil(base, name, expect, classes, change):
    e = dict(base())
    e["wires"], e["consts"] = e["wires"].copy(), e["consts"].copy()
    e.update(name=name, expect=expect, classes=set(classes))
    change(e)
    return e


@_entry
def pair_only_under_the_other_tag():
    """a looking row of table 1 looks up an entry that only table 0 holds: absent under its tag; with word 7 = 0 the pair is there"""
    def change(e):
        i = e["tables"][1][3][-1]
        x, y = e["entries"][0][-1]
        assert (x, y) not in e["entries"][1]
        e["wires"][1 + 2 * 2][i], e["wires"][2 + 2 * 2][i] = x, y
    return _spoil(n8_D2_straddle_C8_shared, "pair_only_under_the_other_tag", "absent", {"other_tag_only"}, change)


@_entry
def tag_flipped_on_a_looking_row():
    """one looking row of table 0 carries tag 1: its slot 0 (the shared entry) is still found, under the other tag; its other pairs
    are not in table 1"""
    def change(e):
        e["consts"][e["desc"][7]][e["tables"][0][3][0]] = e["tables"][1][0]
    return _spoil(n8_D2_straddle_C8_shared, "tag_flipped_on_a_looking_row", "absent", {"tag_flipped"}, change)


SPOILED = [pair_only_under_the_other_tag, tag_flipped_on_a_looking_row]
IDS = [f.__name__ for f in ENTRIES]
BY_NAME = {f.__name__: f for f in ENTRIES + SPOILED}
GOOD_AFTER_REFUSAL = "n8_D2_straddle_C8_shared"
EDGE_CLASSES = {"n4_single_rows", "groups_straddle", "eight_challenges", "same_pair_under_both_tags", "tags_ge_2_63", "tag_words_plus_p",
                "three_tables", "several_blocks", "row0_marked", "last_row_marked", "other_tag_only", "tag_flipped"}

# word 7 on lc.REFUSAL_SHAPE (8 wires, 8 constants, 2 selector columns): (name, description, code or None = served)
TAG_WORDS = [
    ("tag_column_is_a_selector", lc.GOOD_DESC[:7] + (1,), E_BADARG),
    ("second_tag_column_outside", lc.GOOD_DESC[:7] + (7,), E_BADARG),
    ("tag_columns_outside", lc.GOOD_DESC[:7] + (8,), E_BADARG),
    ("tag_word_huge", lc.GOOD_DESC[:7] + (0xFFFFFFFF,), E_BADARG),
    ("empty_description_with_tags", (0, 0, 0, 0, 0, 0, 0, 6), E_BADARG),
    ("first_column_behind_the_selectors", lc.GOOD_DESC[:7] + (2,), None),
    ("last_two_columns", lc.GOOD_DESC[:7] + (6,), None),
]


# ---- whole proofs ----------------------------------------------------------------------------------------------------------------------
PROOF_ENTRY = "n1024_D8_two_tables"


def read_proof(proof, e, challenger):
    """lc.read_proof for a tagged entry: the same layout and transcript; the lookup terms take eta^2 tag from the opened tag columns"""
    saved = lc.lookup_terms_at_zeta
    lc.lookup_terms_at_zeta = lookup_terms_at_zeta
    try:
        return lc.read_proof(proof, e, challenger)
    finally:
        lc.lookup_terms_at_zeta = saved


def lookup_terms_at_zeta(desc, D, C, cv, wv, ss, us, ss_next, l0, etas, thetas):
    q_look, lw, n_look, q_tab, tc, tm, n_tab, t0 = unpack(desc)
    gs = group_slots(desc, D)
    J = len(gs)
    out = [lc.e2_mul(l0, ss[c]) for c in range(C)]
    for c in range(C):
        eta, theta = etas[c] % P, thetas[c] % P
        chain = [ss[c]] + [us[c * (J - 1) + j] for j in range(J - 1)] + [ss_next[c]]
        for j, (looking, slots) in enumerate(gs):
            tag = (cv[t0] if looking else cv[t0 + 1]) if t0 else (0, 0)
            ds = []
            for k in slots:
                vx, vy = (wv[lw + 2 * k], wv[lw + 2 * k + 1]) if looking else (cv[tc + 2 * k], cv[tc + 2 * k + 1])
                comb = lc.e2_add(lc.e2_add(vx, lc.e2_scale(vy, eta)), lc.e2_scale(tag, eta * eta % P))
                ds.append((lc.e2_sub((theta, 0), comb), (1, 0) if looking else wv[tm + k]))
            prod, num = (1, 0), (0, 0)
            for k, (d, m) in enumerate(ds):
                prod = lc.e2_mul(prod, d)
                others = m
                for k2, (d2, _) in enumerate(ds):
                    if k2 != k:
                        others = lc.e2_mul(others, d2)
                num = lc.e2_add(num, others)
            sd = lc.e2_mul(lc.e2_sub(chain[j + 1], chain[j]), prod)
            out.append(lc.e2_sub(sd, lc.e2_mul(cv[q_look], num)) if looking else lc.e2_add(sd, lc.e2_mul(cv[q_tab], num)))
    return out


def tag_opening(e):
    """the word index of the opened looking-tag column's c0 in a flat proof of the zero-constraint circuit over e"""
    return 24 + 12 * (1 << lc.PROOF_FRI["cap_height"]) + 8 + 2 * int(e["desc"][7])


# ---- SIPP_GEN_LOOKUP ---------------------------------------------------------------------------------------------------------------------
GEN_LOOKUP = 17
OTHER = 0xFFFF                      # the selector value of rows no generator takes
SENTINEL = 0xDEADBEEF


def generate(wires, consts, gens, rows=None):
    """the rule of include/sipp_hip.h in plain integers, for every generator (kind 17, selector column, selector value, look_wire0,
    n_look, tab_const0, n_tab, base_col) on every row (of `rows`) that holds it -> (the wire table afterwards, the mask of written
    cells)"""
    out = np.array(wires, dtype=np.uint64).copy()
    written = np.zeros(out.shape, dtype=bool)
    for kind, sel, val, lw, n_look, tc, n_tab, base in gens:
        if kind != GEN_LOOKUP:
            continue
        n = out.shape[1]
        for i in (range(n) if rows is None else rows):
            if int(consts[sel][i]) != val:
                continue
            row0, T = int(consts[base][i]) % P, int(consts[base + 1][i]) % P
            if T == 0:
                continue
            for k in range(n_look):
                x = int(out[lw + 2 * k][i]) % P
                row = row0 + x // n_tab
                y = int(consts[tc + 2 * (x % n_tab) + 1][row]) % P if x < T and row < n else 0
                out[lw + 2 * k + 1][i] = y
                written[lw + 2 * k + 1][i] = True
    return out, written


def dense_table(consts, tc, n_tab, row0, values):
    """entry t = (t, values[t]) in row row0 + t // n_tab, slot t % n_tab; the slots the last row has left repeat the last entry"""
    rows = -(-len(values) // n_tab)
    for s in range(rows * n_tab):
        t = min(s, len(values) - 1)
        consts[tc + 2 * (s % n_tab)][row0 + s // n_tab], consts[tc + 2 * (s % n_tab) + 1][row0 + s // n_tab] = t, values[t]


GEN_K = 12                          # constant columns of the generator instances: selector, c0, c1, then 3 table slots at 3, filler
GEN_SHAPE = (1, 2, 3, 3, 1)         # look_wire0, n_look, tab_const0, n_tab, base_col: wires 1 .. 4, constants 3 .. 8, c0 = 1, c1 = 2


@_entry
def gen_n8():
    """N = 8, n_tab = 3, two looking slots.  Table f: T = 7 entries from row 0 (rows 0, 1, 2; the last row padded), values above 2^63
    and one given as value + p.  Table g: T = 4 entries from row 6 (rows 6, 7): its entry 6 would sit in row 8 = N.  Looking rows: 3
    (f: x = 0 and T - 1), 4 (f: x = T and x = 3 + p), 5 (g: x = 3; x = 6 < its claimed T = 9 in a row outside the circuit), 2 is a
    T = 0 row that is ALSO a table row of f.  Row 4's c0 = row0 is given as 0 + p."""
    rng = np.random.default_rng(41)
    n, W = 8, 6
    consts, wires = lc._rand(rng, (GEN_K, n)), lc._rand(rng, (W, n))
    consts[0] = OTHER
    f = [(1 << 63) + 11, 5, 0, P - 1, 17 + P, 1, (1 << 63) + 3]
    g = [9, 8, 7, 6]
    dense_table(consts, 3, 3, 0, f)
    dense_table(consts, 3, 3, 6, g)
    for i, c0, c1, xs in ((3, 0, 7, (0, 6)), (4, P, 7, (7, 3 + P)), (5, 6, 9, (3, 6)), (2, 0, 0, (1, 2))):
        consts[0][i], consts[1][i], consts[2][i] = 1, c0, c1
        for k, x in enumerate(xs):
            wires[1 + 2 * k][i], wires[2 + 2 * k][i] = x, SENTINEL
    return _gen_entry("gen_n8", 3, wires, consts, [(GEN_LOOKUP, 0, 1) + GEN_SHAPE], None)


@_entry
def gen_n8_chain():
    """three levels: y1 = f(x) on row 3, copied into the x of row 4, y2 = g(y1) there, copied into row 5 whose x = y2 is looked up in f
    again.  f = t -> 6 - t (T = 7, row 0), g = t -> (3 t) mod 7 (T = 7, row 5 .. 7: its table rows are also looking rows' neighbours)"""
    rng = np.random.default_rng(42)
    n, W = 8, 6
    consts, wires = lc._rand(rng, (GEN_K, n)), lc._rand(rng, (W, n))
    consts[0] = OTHER
    dense_table(consts, 3, 3, 0, [6 - t for t in range(7)])
    dense_table(consts, 3, 3, 5, [3 * t % 7 for t in range(7)])
    for i, c0 in ((3, 0), (4, 5), (6, 0)):
        consts[0][i], consts[1][i], consts[2][i] = 1, c0, 7
        wires[1:5, i] = SENTINEL
    wires[1][3], wires[3][3] = 2, 5
    cell = lambda w, r: w * n + r
    sched = {"n_levels": 3, "rows": np.array([3, 4, 6], dtype=np.uint32), "level_offsets": np.array([0, 1, 2, 3], dtype=np.uint32),
             "copy_src": np.array([cell(2, 3), cell(4, 3), cell(2, 4), cell(4, 4)], dtype=np.uint64),
             "copy_dst": np.array([cell(1, 4), cell(3, 4), cell(1, 6), cell(3, 6)], dtype=np.uint64),
             "copy_offsets": np.array([0, 2, 4, 4], dtype=np.uint32)}
    return _gen_entry("gen_n8_chain", 3, wires, consts, [(GEN_LOOKUP, 0, 1) + GEN_SHAPE], sched)


@_entry
def gen_wide_level():
    """N = 2^14 rows in ONE level: the size at which sipp_plonk_generate_witness_levels runs one lane per row (plonk_witness_level_kernel).
    A 256-entry table from row 100; every other row from 1000 on is a looking row with random x below 300 (some outside T = 256)"""
    rng = np.random.default_rng(43)
    n, W = 1 << 14, 6
    consts, wires = lc._rand(rng, (GEN_K, n)), lc._rand(rng, (W, n))
    consts[0] = OTHER
    dense_table(consts, 3, 3, 100, [int(v) for v in lc._rand(rng, (256,))])
    rows = np.arange(1000, n, 2)
    consts[0][rows], consts[1][rows], consts[2][rows] = 1, 100, 256
    wires[1][rows] = rng.integers(0, 300, size=len(rows), dtype=np.uint64)
    wires[3][rows] = rng.integers(0, 300, size=len(rows), dtype=np.uint64)
    wires[2][rows], wires[4][rows] = SENTINEL, SENTINEL
    sched = {"n_levels": 1, "rows": np.arange(n, dtype=np.uint32)[::-1].copy(), "level_offsets": np.array([0, n], dtype=np.uint32),
             "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64), "copy_offsets": np.array([0, 0], dtype=np.uint32)}
    return _gen_entry("gen_wide_level", 14, wires, consts, [(GEN_LOOKUP, 0, 1) + GEN_SHAPE], sched)


def _gen_entry(name, log_n, wires, consts, gens, sched):
    w = wires.copy()
    written = np.zeros(w.shape, dtype=bool)
    if sched is None:
        expected, written = generate(w, consts, gens)
    else:       # level by level: the level's rows, then its copies
        flat = w.reshape(-1)
        for l in range(sched["n_levels"]):
            w, wr = generate(w, consts, gens, [int(r) for r in sched["rows"][sched["level_offsets"][l]:sched["level_offsets"][l + 1]]])
            written |= wr
            flat = w.reshape(-1)
            for s, d in zip(sched["copy_src"][sched["copy_offsets"][l]:sched["copy_offsets"][l + 1]],
                            sched["copy_dst"][sched["copy_offsets"][l]:sched["copy_offsets"][l + 1]]):
                flat[int(d)] = flat[int(s)]
                written.reshape(-1)[int(d)] = True
        expected = w
    return dict(name=name, log_n=log_n, wires=wires, consts=consts, gens=gens, sched=sched, expected=expected, written=written)


GEN_ENTRIES = [gen_n8, gen_n8_chain, gen_wide_level]
BY_NAME_GEN = {f.__name__: f for f in GEN_ENTRIES}
# layouts witness_prepare refuses, on 6 wires and GEN_K = 12 constants: (name, (look_wire0, n_look, tab_const0, n_tab, base_col))
GEN_REFUSALS = [("n_look_0", (1, 0, 3, 3, 1)), ("n_tab_0", (1, 2, 3, 0, 1)), ("looking_wires_run_outside", (3, 2, 3, 3, 1)),
                ("look_wire0_huge", (0xFFFFFFFF, 2, 3, 3, 1)), ("table_columns_run_outside", (1, 2, 7, 3, 1)),
                ("n_tab_huge", (1, 2, 3, 0x80000000, 1)), ("base_col_last", (1, 2, 3, 3, 11)), ("base_col_huge", (1, 2, 3, 3, 0xFFFFFFFF))]
GEN_SERVED = [("everything_at_its_end", (2, 2, 6, 3, 10))]
