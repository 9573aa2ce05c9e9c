"""A catalogue of lookup instances at the edges of the log-derivative lookup argument (sipp_amd/csrc/lookup.hip: lookup_zero_kernel,
lookup_count_kernel, lookup_group_kernel, lookup_scan_kernel, lookup_u_kernel), built explicitly, with an exact Python-integer reading
of the statement in include/sipp_hip.h: the multiplicities, the running-sum columns S / U, the argument's terms on a row of the
subgroup, and (at the end) the verifier's vanishing equation with the lookup terms over the extension, read from the opened values of
a flat "SIPPPLK4" proof.  CPU only: nothing here touches the GPU, and the library only through the transcript object read_proof() is
handed.  Used by tests/test_lookup_reading.py (the reading against its own statement: the terms vanish on honest instances and catch
spoiled ones; proof that every edge class is reached; the committed proof), tests/test_lookup_builder.py (a CircuitBuilder circuit's
tables) and tests/test_gpu_lookups.py (the device word for word against the reading; whole proofs).

An entry function returns a dict: name, log_n, D (chunk size), C (challenges), num_selectors, desc (the eight description words),
wires [W][N] and consts [K][N] (uint64, as handed to the device: the m cells hold garbage, unmarked rows hold garbage in every column
the argument names), etas, thetas (Python ints, as handed to the device), classes (the edge classes the entry reaches), and `expect`:
"ok", "absent" (a looked-up pair is in no table slot: the multiplicities are refused) or "vanishing" (theta sits on a combination of a
marked row: the sums are refused).  REFUSALS lists descriptions the library refuses before it launches anything, with their codes."""
import functools

import numpy as np

P = 0xFFFFFFFF00000001
E_BADARG, E_UNSUPPORTED, E_WITNESS = -1, -7, -8
MAX_SLOTS = 128


class Absent(Exception):
    """a looked-up pair is in no table slot"""


class Vanishing(Exception):
    """theta - (x + eta y) = 0 on a marked row"""


def _rand(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def groups(slots, D):
    return -(-slots // D)


def unpack(desc):
    q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab, last = [int(x) for x in desc]
    return q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab


# ---- the reading -----------------------------------------------------------------------------------------------------------------------
def multiplicities(desc, wires, consts):
    """the wire table after sipp_plonk_lookup_multiplicities: the m cells of the table rows zeroed, then one added per looking slot to
    the FIRST table slot in (row, slot) order with the equal field pair.  Raises Absent."""
    q_look, lw, n_look, q_tab, tc, tm, n_tab = unpack(desc)
    out = np.array(wires, dtype=np.uint64).copy()
    n = out.shape[1]
    first = {}
    for i in range(n):
        if int(consts[q_tab][i]) % P:
            for k in range(n_tab):
                out[tm + k][i] = 0
                first.setdefault((int(consts[tc + 2 * k][i]) % P, int(consts[tc + 2 * k + 1][i]) % P), (tm + k, i))
    counts = {}
    for i in range(n):
        if int(consts[q_look][i]) % P:
            for k in range(n_look):
                # read from `out`: a looking wire that is also an m cell of a table row is read as zeroed
                key = (int(out[lw + 2 * k][i]) % P, int(out[lw + 2 * k + 1][i]) % P)
                if key not in first:
                    raise Absent((i, k, key))
                counts[first[key]] = counts.get(first[key], 0) + 1
    for (col, i), v in counts.items():
        out[col][i] = v
    return out


def group_slots(desc, D):
    """[(is_looking, [slot, ...]), ...]: the J groups in chain order"""
    _, _, n_look, _, _, _, n_tab = unpack(desc)
    out = [(True, list(range(j * D, min((j + 1) * D, n_look)))) for j in range(groups(n_look, D))]
    return out + [(False, list(range(j * D, min((j + 1) * D, n_tab)))) for j in range(groups(n_tab, D))]


def denominators(desc, wires, consts, i, looking, slots, eta, theta):
    """the d_k (looking) or (e_k, m_k) (table) of a group on row i"""
    _, lw, _, _, tc, tm, _ = unpack(desc)
    if looking:
        return [((theta - (int(wires[lw + 2 * k][i]) + eta * int(wires[lw + 2 * k + 1][i]))) % P, 1) for k in slots]
    return [((theta - (int(consts[tc + 2 * k][i]) + eta * int(consts[tc + 2 * k + 1][i]))) % P, int(wires[tm + k][i]) % P) for k in slots]


def sums(desc, wires, consts, D, etas, thetas):
    """S_0 .. S_(C-1), then U_0 .. U_(J-2) challenge by challenge: [C J][N] uint64.  Raises Vanishing."""
    q_look, _, _, q_tab, _, _, _ = unpack(desc)
    n = np.asarray(wires).shape[1]
    gs = group_slots(desc, D)
    J = len(gs)
    s_cols, u_cols = [], []
    for eta, theta in zip(etas, thetas):
        eta, theta = eta % P, theta % P
        s, us = [], [[] for _ in range(J - 1)]
        acc = 0
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
        s_cols.append(s)
        u_cols += us
        s.append(acc)             # S(g w^(N-1)) = S(1) must be 0 again: kept behind the column for `closes`
    closes = all(col[-1] == 0 for col in s_cols)
    return np.array([col[:n] for col in s_cols] + u_cols, dtype=np.uint64), closes


def terms_on_row(desc, wires, consts, D, cols, C, c, eta, theta, i):
    """the J + 1 terms of challenge c at x = w^i from the columns: L_0(x) S(x), then per group
    (U_j - U_(j-1)) Dl - q_look Nl  or  (U_j - U_(j-1)) Dt + q_tab Nt,  U_(-1) = S(x), U_(J-1) = S(g x)"""
    q_look, _, _, q_tab, _, _, _ = unpack(desc)
    n = np.asarray(wires).shape[1]
    gs = group_slots(desc, D)
    J = len(gs)
    eta, theta = eta % P, theta % P
    chain = [int(cols[c][i])] + [int(cols[C + c * (J - 1) + j][i]) for j in range(J - 1)] + [int(cols[c][(i + 1) % n])]
    out = [int(cols[c][i]) if i == 0 else 0]
    for j, (looking, slots) in enumerate(gs):
        ds = denominators(desc, wires, consts, i, looking, slots, eta, theta)
        prod, num = 1, 0
        for k, (d, m) in enumerate(ds):
            prod = prod * d % P
            others = 1
            for k2, (d2, _) in enumerate(ds):
                if k2 != k:
                    others = others * d2 % P
            num = (num + m * others) % P
        q = int(consts[q_look if looking else q_tab][i]) % P
        step = (chain[j + 1] - chain[j]) % P
        out.append((step * prod - q * num) % P if looking else (step * prod + q * num) % P)
    return out


def all_terms_vanish(e, wires, cols):
    n = 1 << e["log_n"]
    return all(t == 0 for c in range(e["C"]) for i in range(n)
               for t in terms_on_row(e["desc"], wires, e["consts"], e["D"], cols, e["C"], c, e["etas"][c], e["thetas"][c], i))


def first_mismatch(got, want):
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    col, row = bad[0]
    return "%d cells differ; first at column %d row %d: %#x, expected %#x" % (len(bad), col, row, int(got[col][row]), int(want[col][row]))


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------
def build(name, log_n, D, C, n_look, n_tab, table_rows, look_rows, seed, *, pad=0, hit="spread", big_keys=False, plus_p=False,
          wire_pad=1, const_pad=0, classes=()):
    """One instance.  Constants: column 0 the selector, then `const_pad` filler columns, q_look, q_tab, the 2 n_tab table columns.
    Wires: `wire_pad` filler columns, the 2 n_look looking wires, the n_tab multiplicity wires.  The table's real entries are distinct
    pairs; the last `pad` slots of the last table row repeat earlier entries.  hit: "spread" = looks drawn from the first half of the
    entries (the rest is never hit), "one" = every looking slot hits one entry, "dups" = looks drawn from the repeated entries."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    q_look, q_tab = 1 + const_pad, 2 + const_pad
    tab_const0 = q_tab + 1
    K, W = tab_const0 + 2 * n_tab, wire_pad + 2 * n_look + n_tab
    look_wire0, tab_mult0 = wire_pad, wire_pad + 2 * n_look
    desc = (q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab, 0)
    consts, wires = _rand(rng, (K, n)), _rand(rng, (W, n))
    consts[0] = 0
    consts[q_look], consts[q_tab] = 0, 0
    consts[q_look][list(look_rows)] = 1
    consts[q_tab][list(table_rows)] = 1
    n_real = len(table_rows) * n_tab - pad
    assert n_real >= 1
    entries = []
    while len(entries) < n_real:
        x, y = int(_rand(rng, ())), int(_rand(rng, ()))
        if big_keys:
            x, y = (1 << 63) + (x >> 2), (1 << 63) + (y >> 2)              # canonical: below 2^63 + 2^62 < p
        else:
            x, y = x & 0xFFFF, (y & 0xFF) if len(entries) % 3 else 0      # small, so that x + p fits a word
        if (x, y) not in entries:
            entries.append((x, y))
    slots = entries + [entries[int(rng.integers(0, min(n_real, max(1, pad))))] for _ in range(pad)]
    repeated = sorted(set(slots[n_real:]))
    for t, (x, y) in enumerate(slots):
        i, k = table_rows[t // n_tab], t % n_tab
        consts[tab_const0 + 2 * k][i], consts[tab_const0 + 2 * k + 1][i] = x, y
    pool = {"spread": entries[: max(1, n_real // 2)], "one": entries[-1:], "dups": repeated or entries[:1]}[hit]
    for i in look_rows:
        for k in range(n_look):
            x, y = pool[int(rng.integers(0, len(pool)))]
            if plus_p and (i + k) % 2 == 0 and x + P < 1 << 64 and y + P < 1 << 64:
                x, y = x + P, y + P                                         # the same field pair in other words
            wires[look_wire0 + 2 * k][i], wires[look_wire0 + 2 * k + 1][i] = x, y
    etas, thetas = [int(v) for v in _rand(rng, (C,))], [int(v) for v in _rand(rng, (C,))]
    if plus_p:
        etas[0], thetas[0] = (etas[0] & 0xFFFFFFF) + P, (thetas[0] & 0xFFFFFFF) + P
    return dict(name=name, log_n=log_n, D=D, C=C, num_selectors=1, desc=desc, wires=wires, consts=consts, etas=etas, thetas=thetas,
                classes=set(classes), expect="ok", table_rows=list(table_rows), look_rows=list(look_rows), entries=entries,
                repeated=repeated)


def _entry(fn):
    return functools.lru_cache(maxsize=None)(fn)


@_entry
def n4_one_table_row_one_looking_row():
    return build("n4_one_table_row_one_looking_row", 2, 2, 1, 1, 1, [2], [1], 11, hit="one", classes={"n4_single_rows", "one_entry"})


@_entry
def n8_D2_look_D_tab_Dp1():
    return build("n8_D2_look_D_tab_Dp1", 3, 2, 2, 2, 3, [0, 5], [1, 2, 7], 12, pad=1, classes={"padded_duplicates", "never_hit", "row0_marked"})


@_entry
def n32_D4_look_Dp1_tab_1():
    return build("n32_D4_look_Dp1_tab_1", 5, 4, 2, 5, 1, list(range(8, 20)), [0, 3, 31], 13, const_pad=2, wire_pad=3,
                 classes={"never_hit", "last_row_marked"})


@_entry
def n64_D4_C8_look_2Dp3_tab_Dp1():
    return build("n64_D4_C8_look_2Dp3_tab_Dp1", 6, 4, 8, 11, 5, [1, 2, 3, 60], list(range(10, 50, 3)), 14, pad=3, hit="dups",
                 classes={"padded_duplicates", "looks_on_duplicates", "eight_challenges"})


@_entry
def n1024_D8_look_2Dp3_tab_Dp1():
    return build("n1024_D8_look_2Dp3_tab_Dp1", 10, 8, 2, 19, 9, list(range(0, 1024, 37)), list(range(5, 1024, 11)), 15, pad=4,
                 classes={"padded_duplicates", "never_hit", "several_blocks", "row0_marked"})


@_entry
def n1024_D8_every_slot_hits_one_entry():
    return build("n1024_D8_every_slot_hits_one_entry", 10, 8, 1, 8, 1, list(range(100, 140)), list(range(200, 1024)), 16, hit="one",
                 classes={"one_entry", "never_hit", "several_blocks"})


@_entry
def n16_D2_keys_above_2_63():
    return build("n16_D2_keys_above_2_63", 4, 2, 1, 7, 3, [4, 9], [0, 1, 2, 15], 17, big_keys=True, classes={"keys_ge_2_63", "never_hit"})


@_entry
def n32_D8_C8_words_plus_p():
    return build("n32_D8_C8_words_plus_p", 5, 8, 8, 1, 9, [7, 8], [7, 20, 21], 18, pad=2, plus_p=True,
                 classes={"words_plus_p", "row_both_table_and_looking", "padded_duplicates", "eight_challenges"})


@_entry
def n256_D8_look_Dp1():
    return build("n256_D8_look_Dp1", 8, 8, 2, 9, 1, list(range(64, 128)), list(range(0, 256, 5)), 19, classes={"never_hit", "row0_marked"})


@_entry
def n2048_D2_scan_two_rows_a_thread():
    """2^11 rows: the one size here at which the scan gives every thread more than one row"""
    return build("n2048_D2_scan_two_rows_a_thread", 11, 2, 1, 1, 1, list(range(1, 2048, 2)), list(range(0, 2048, 2)), 20,
                 classes={"scan_several_rows_a_thread", "several_blocks", "row0_marked"})


def _spoil(base, name, expect, classes, change):
    e = dict(base())
    e["wires"], e["consts"] = e["wires"].copy(), e["consts"].copy()
    e["etas"], e["thetas"] = list(e["etas"]), list(e["thetas"])
    e.update(name=name, expect=expect, classes=set(classes))
    change(e)
    return e


@_entry
def absent_pair():
    def change(e):
        _, lw, n_look, _, _, _, _ = unpack(e["desc"])
        i = e["look_rows"][-1]
        x = int(e["wires"][lw + 2 * (n_look - 1)][i])
        e["wires"][lw + 2 * (n_look - 1)][i] = (x + 0x10000) % P          # no entry has an x this large: the last slot of the last looking row
    return _spoil(n64_D4_C8_look_2Dp3_tab_Dp1, "absent_pair", "absent", {"absent_pair"}, change)


@_entry
def theta_on_a_looking_combination():
    def change(e):
        _, lw, n_look, _, _, _, _ = unpack(e["desc"])
        i, k, c = e["look_rows"][1], n_look - 1, e["C"] - 1
        e["thetas"][c] = (int(e["wires"][lw + 2 * k][i]) + e["etas"][c] * int(e["wires"][lw + 2 * k + 1][i])) % P
    return _spoil(n32_D4_look_Dp1_tab_1, "theta_on_a_looking_combination", "vanishing", {"theta_on_looking"}, change)


@_entry
def theta_on_a_table_combination():
    def change(e):
        _, _, _, _, tc, _, n_tab = unpack(e["desc"])
        i, k, c = e["table_rows"][0], n_tab - 1, 0
        e["thetas"][c] = (int(e["consts"][tc + 2 * k][i]) + e["etas"][c] * int(e["consts"][tc + 2 * k + 1][i])) % P
    return _spoil(n8_D2_look_D_tab_Dp1, "theta_on_a_table_combination", "vanishing", {"theta_on_table"}, change)


ENTRIES = [n4_one_table_row_one_looking_row, n8_D2_look_D_tab_Dp1, n32_D4_look_Dp1_tab_1, n64_D4_C8_look_2Dp3_tab_Dp1,
           n1024_D8_look_2Dp3_tab_Dp1, n1024_D8_every_slot_hits_one_entry, n16_D2_keys_above_2_63, n32_D8_C8_words_plus_p,
           n256_D8_look_Dp1, n2048_D2_scan_two_rows_a_thread]
SPOILED = [absent_pair, theta_on_a_looking_combination, theta_on_a_table_combination]
IDS = [f.__name__ for f in ENTRIES]
SPOILED_IDS = [f.__name__ for f in SPOILED]
BY_NAME = {f.__name__: f for f in ENTRIES + SPOILED}
GOOD_AFTER_REFUSAL = "n8_D2_look_D_tab_Dp1"
EDGE_CLASSES = {"n4_single_rows", "one_entry", "never_hit", "padded_duplicates", "looks_on_duplicates", "keys_ge_2_63", "words_plus_p",
                "absent_pair", "theta_on_looking", "theta_on_table", "several_blocks", "scan_several_rows_a_thread", "eight_challenges",
                "row_both_table_and_looking", "row0_marked", "last_row_marked"}

# descriptions refused before anything is launched, on a circuit of 8 wires, 8 constants, 2 selector columns:
# (name, (q_look, look_wire0, n_look, q_tab, tab_const0, tab_mult0, n_tab, last), code)
REFUSAL_SHAPE = dict(log_n=3, num_wires=8, num_constants=8, num_selectors=2, D=2, C=1)
GOOD_DESC = (2, 0, 2, 3, 4, 4, 2, 0)
REFUSALS = [
    ("q_look_outside", (8, 0, 2, 3, 4, 4, 2, 0), E_BADARG),
    ("q_tab_outside", (2, 0, 2, 8, 4, 4, 2, 0), E_BADARG),
    ("looking_wires_run_outside", (2, 5, 2, 3, 4, 4, 2, 0), E_BADARG),
    ("look_wire0_huge", (2, 0xFFFFFFFF, 2, 3, 4, 4, 2, 0), E_BADARG),
    ("table_constants_run_outside", (2, 0, 2, 3, 5, 4, 2, 0), E_BADARG),
    ("multiplicity_wires_run_outside", (2, 0, 2, 3, 4, 7, 2, 0), E_BADARG),
    ("q_look_is_a_selector", (1, 0, 2, 3, 4, 4, 2, 0), E_BADARG),
    ("q_tab_is_a_selector", (2, 0, 2, 0, 4, 4, 2, 0), E_BADARG),
    ("looks_without_table", (2, 0, 2, 3, 4, 4, 0, 0), E_BADARG),
    ("table_without_looks", (2, 0, 0, 3, 4, 4, 2, 0), E_BADARG),
    ("last_word_not_zero", (2, 0, 2, 3, 4, 4, 2, 1), E_BADARG),
    ("n_look_129", (2, 0, 129, 3, 4, 4, 2, 0), E_UNSUPPORTED),
    ("n_tab_129", (2, 0, 2, 3, 4, 4, 129, 0), E_UNSUPPORTED),
]
# served on the same circuit, one step inside a refusal above: look_wire0 + 2 n_look == num_wires (looking_wires_run_outside is one past)
SERVED_AT_THE_EDGE = [
    ("looking_wires_end_at_the_last_wire", (2, 4, 2, 3, 4, 4, 2, 0)),
]


# ---- whole proofs: the shape, and the verifier's vanishing equation read from the opened values ------------------------------------------
# One circuit carries the catalogue's tables through the prover: every row is the same gate without constraints (selector column 0
# holds its index, 0), the first PROOF_ROUTED wires are routed with the identity permutation.  The vanishing polynomial is then the
# permutation's terms and the lookup argument's, nothing else, and the reading below checks the WHOLE equation at zeta.
PROOF_ENTRY = "n1024_D8_look_2Dp3_tab_Dp1"
PROOF_ROUTED = 4
PROOF_FRI = dict(rate_bits=3, cap_height=4, pow_bits=8, num_queries=8)
PROOF_DIGEST = (17, 0, P - 1, 1 << 32)
ROOT32 = 1753635133440165772            # a primitive 2^32-th root of unity


def proof_circuit(e):
    """the circuit dict (sipp_amd.PlonkCircuit.from_dict) of the zero-constraint circuit over entry e"""
    return {"num_wires": int(e["wires"].shape[0]), "num_routed": PROOF_ROUTED, "num_constants": int(e["consts"].shape[0]), "num_selectors": 1,
            "gates": [(0, 0, 0, 1, 0, 0)], "programs": np.zeros(0, dtype=np.int64)}


def constants_sigmas(e):
    """[K + R][N]: the entry's constant columns, then identity sigmas sigma_j(i) = 7^j w^i"""
    n = 1 << e["log_n"]
    w = pow(ROOT32, 1 << (32 - e["log_n"]), P)
    x, acc = [], 1
    for _ in range(n):
        x.append(acc)
        acc = acc * w % P
    sig = [[pow(7, j, P) * xi % P for xi in x] for j in range(PROOF_ROUTED)]
    return np.concatenate([np.asarray(e["consts"], dtype=np.uint64), np.array(sig, dtype=np.uint64)])


def e2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e2_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)       # X^2 = 7


def e2_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def e2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = e2_mul(r, a)
        a = e2_mul(a, a)
        e >>= 1
    return r


def e2_inv(a):
    norm = (a[0] * a[0] - 7 * a[1] * a[1]) % P
    ni = pow(norm, -1, P)
    return (a[0] * ni % P, (-a[1]) * ni % P)


def lookup_terms_at_zeta(desc, D, C, cv, wv, ss, us, ss_next, l0, etas, thetas):
    """the lookup half of the verifier: the C boundary terms L_0(zeta) S_c(zeta), then challenge by challenge the J chain terms, over
    the extension from the opened constants cv, wires wv, S columns ss, U columns us and the S columns at g zeta"""
    q_look, lw, n_look, q_tab, tc, tm, n_tab = unpack(desc)
    gs = group_slots(desc, D)
    J = len(gs)
    out = [e2_mul(l0, ss[c]) for c in range(C)]
    for c in range(C):
        eta, theta = etas[c] % P, thetas[c] % P
        chain = [ss[c]] + [us[c * (J - 1) + j] for j in range(J - 1)] + [ss_next[c]]
        for j, (looking, slots) in enumerate(gs):
            ds = []
            for k in slots:
                vx, vy = (wv[lw + 2 * k], wv[lw + 2 * k + 1]) if looking else (cv[tc + 2 * k], cv[tc + 2 * k + 1])
                ds.append((e2_sub((theta, 0), e2_add(vx, e2_scale(vy, eta))), (1, 0) if looking else wv[tm + k]))
            prod, num = (1, 0), (0, 0)
            for k, (d, m) in enumerate(ds):
                prod = e2_mul(prod, d)
                others = m
                for k2, (d2, _) in enumerate(ds):
                    if k2 != k:
                        others = e2_mul(others, d2)
                num = e2_add(num, others)
            sd = e2_mul(e2_sub(chain[j + 1], chain[j]), prod)
            out.append(e2_sub(sd, e2_mul(cv[q_look], num)) if looking else e2_add(sd, e2_mul(cv[q_tab], num)))
    return out


def read_proof(proof, e, challenger):
    """a flat "SIPPPLK4" proof of the zero-constraint circuit over entry e (no public inputs) -> the first stage that fails, or None:
    "header", "vanishing".  `challenger`: a fresh transcript object with observe(word) and get() (the library's host challenger)."""
    pf = [int(v) for v in proof]
    desc, D, C, log_n = e["desc"], e["D"], e["C"], e["log_n"]
    K, W, R = int(e["consts"].shape[0]), int(e["wires"].shape[0]), PROOF_ROUTED
    m = -(-R // D)
    npp = m - 1
    J = len(group_slots(desc, D))
    nz, nlk = C * m, C * J
    n_cap = 1 << PROOF_FRI["cap_height"]
    hw = 24
    if len(pf) < hw + 12 * n_cap + 8 or pf[0] != int.from_bytes(b"SIPPPLK4", "little") or pf[1:5] != [log_n, R, D, C] or pf[5] != len(pf):
        return "header"
    if pf[6:12] != [W, K, 1, 1, 0, 0] or any(pf[12:16]) or pf[16:24] != [int(x) for x in desc]:
        return "header"
    caps = [pf[hw + 4 * n_cap * o: hw + 4 * n_cap * (o + 1)] for o in range(3)]
    at = hw + 12 * n_cap + 8
    n0 = K + R + W + nz + nlk + C * D
    n_open = n0 + 2 * C
    if len(pf) < at + 2 * n_open:
        return "header"
    v = [(pf[at + 2 * k], pf[at + 2 * k + 1]) for k in range(n_open)]
    cv, sg, wv = v[:K], v[K:K + R], v[K + R:K + R + W]
    zs = v[K + R + W:]
    pps, ss, us, qs = zs[C:nz], zs[nz:nz + C], zs[nz + C:nz + nlk], zs[nz + nlk:nz + nlk + C * D]
    zs_next, ss_next = v[n0:n0 + C], v[n0 + C:]
    ch = challenger
    for wd in list(PROOF_DIGEST) + [0, 0, 0, 0] + caps[0]:      # hash_no_pad of no public inputs: four zero words
        ch.observe(wd)
    betas, gammas = [ch.get() for _ in range(C)], [ch.get() for _ in range(C)]
    etas, thetas = [ch.get() for _ in range(C)], [ch.get() for _ in range(C)]
    for wd in caps[1]:
        ch.observe(wd)
    alphas = [ch.get() for _ in range(C)]
    for wd in caps[2]:
        ch.observe(wd)
    zeta = (ch.get(), ch.get())
    n = 1 << log_n
    zeta_n = e2_pow(zeta, n)
    zh = e2_sub(zeta_n, (1, 0))
    l0 = e2_mul(zh, e2_inv(e2_scale(e2_sub(zeta, (1, 0)), n)))
    terms = [e2_mul(l0, e2_sub(zs[c], (1, 0))) for c in range(C)]
    for c in range(C):
        for q in range(m):
            num = den = (1, 0)
            for j in range(q * D, min((q + 1) * D, R)):
                g = (gammas[c], 0)
                num = e2_mul(num, e2_add(e2_add(wv[j], e2_scale(zeta, betas[c] * pow(7, j, P) % P)), g))
                den = e2_mul(den, e2_add(e2_add(wv[j], e2_scale(sg[j], betas[c])), g))
            prev = zs[c] if q == 0 else pps[c * npp + q - 1]
            nxt = zs_next[c] if q == npp else pps[c * npp + q]
            terms.append(e2_sub(e2_mul(prev, num), e2_mul(nxt, den)))
    terms += lookup_terms_at_zeta(desc, D, C, cv, wv, ss, us, ss_next, l0, etas, thetas)
    for c in range(C):
        van = (0, 0)
        for t in reversed(terms):
            van = e2_add(e2_scale(van, alphas[c]), t)
        acc = (0, 0)
        for d in reversed(range(D)):
            acc = e2_add(e2_mul(acc, zeta_n), qs[c * D + d])
        if van != e2_mul(zh, acc):
            return "vanishing"
    return None
