"""A catalogue of wire tables at the value and layout edges of the outer prover's witness generators (sipp_plonk_generate_witness and
sipp_plonk_generate_witness_levels, sipp_amd/csrc/witness.hip), with an exact reference of the nine families.

THE REFERENCE is written from the SIPP_GEN_* table of include/sipp_hip.h over Python integers (`%` on ints, pow(x, 7, p)); Poseidon is the
naive 30-round form with the constants of data/poseidon_goldilocks_rc.txt.  It shares no code with oracle/plonk_witness.c,
tools/plonk_synth.py, tests/_merkle_reading.py or sipp_amd/merkle.py: those are the readings the CPU test holds it against.  Per family
three small functions: reads(g) (the wires and constant columns a row's generator reads), writes(g) (the wires it writes) and compute(g, ..)
(the written values in the order of writes(g)).  generate() runs a generator list row-locally or replays a level schedule (per level the
generators of its rows in list order, then the copies); every distinct input tuple is evaluated once and tiled over the rows that hold it.

AN ENTRY is a dict: name, log_n, num_wires, num_constants, wires (the INPUT table: generated cells hold SENTINEL, rows of the selector
value OTHER and cells no generator touches hold random field elements), consts (column 0 = the selector, 1 .. 7 constants), pih, gens
[(kind, selector_index, row, p0 .. p4)], sched (None = row-local), expected, written (mask of the cells a generator or a copy writes),
kind (the family of every row, 0 = none), paths (the launch paths that take it: plan()), crafted [(row, output)] (Poseidon rows built to
carry in that output of the first MDS layer).

The value lattice is _gate_edges.EDGE_VALUES = (0, 1, p - 1, 2^32 - 1, 2^32, p - 2^32), MORE adds p - 2, 2^63, 2^32 + 1.

THE CARRY.  witness.hip's MDS layers accumulate 32-bit halves exactly (al, ah), form lo = al + (ah << 32), hi = (ah >> 32) + (lo < al) and
reduce hi 2^64 + lo.  lo < al needs ah mod 2^32 within ~255 of 2^32: about 3e-8 per output on uniform states.  crafted_state() forces it: 7 is
invertible mod p - 1, so the state after round 0's S-boxes can be chosen freely (input = root7(target) - rc_0); all low halves of the
target are 0xFFFFFFFF and the high half of one element with an odd coefficient is solved so that ah mod 2^32 = 2^32 - 3 in the designated
output.  For every output two states: the solved element on the matrix diagonal (c = r; for r = 0 its coefficient holds the +8 of the
diagonal term) and off it."""
import functools
import itertools
import os

import numpy as np

from tests import _gate_edges

P = 2 ** 64 - 2 ** 32 + 1
M32 = 0xFFFFFFFF
EDGE = _gate_edges.EDGE_VALUES
MORE = EDGE + (P - 2, 1 << 63, (1 << 32) + 1)
SENTINEL = 0xDEADBEEF
OTHER = 0xFFFF                      # selector value of the rows no generator takes
NUM_CONSTANTS, C0, C1 = 8, 1, 2     # column 0 selects; the arithmetic generators read columns 1 and 2, the constant ones 1 .. 7
PIH_A, PIH_B = (0, P - 1, M32, 1 << 32), (P - (1 << 32), 1, 1 << 63, P - 2)
ARITHMETIC, BASE_SPLIT, CONSTANT, PUBLIC_INPUT, U32_MUL_ADD, RANDOM_ACCESS, REDUCING, POSEIDON, POSEIDON_SWAP = range(1, 10)
FAMILY = ["none", "ARITHMETIC", "BASE_SPLIT", "CONSTANT", "PUBLIC_INPUT", "U32_MUL_ADD", "RANDOM_ACCESS", "REDUCING", "POSEIDON", "POSEIDON_SWAP"]
COOP_BELOW_ROWS = 16384             # sipp_plonk_generate_witness_levels: a level of fewer rows runs sixteen lanes per row

# layouts of the Poseidon families: upstream's (in 0, out 12, swap 24, delta 25, sbox 29), the shifted one of test_gpu_merkle_circuit.py,
# and one whose last S-box wire is wire 169 of a 170-wire table; plain Poseidon in 136 wires is tools/plonk_synth's (0, 12, 24)
SWAP_LAYOUTS = {"upstream": (135, dict(in_=0, out=12, swap=24, delta=25, sbox=29)),
                "shifted": (170, dict(in_=40, out=5, swap=17, delta=0, sbox=60)),
                "last": (170, dict(in_=20, out=0, swap=33, delta=34, sbox=64))}
PLAIN_LAYOUTS = {"upstream": (136, dict(in_=0, out=12, sbox=24)),
                 "shifted": (170, dict(in_=40, out=5, sbox=60)),
                 "last": (170, dict(in_=20, out=0, sbox=64))}


def _rc():
    vals = []
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "poseidon_goldilocks_rc.txt")) as f:
        for line in f:
            vals += [int(t, 16) for t in line.split("#")[0].replace(",", " ").split()]
    assert len(vals) == 360
    return vals


RC = _rc()
_CIRC = (17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20)
MDS = [[_CIRC[(c - r) % 12] + (8 if r == c == 0 else 0) for c in range(12)] for r in range(12)]


# ------------------------------------------------------------------------------------------------------------------------ the reference
def permutation(state):
    """(the 106 S-box inputs of rounds 1 .. 29 in wire order, the 12 outputs) of the naive permutation"""
    s, sbox = [int(x) % P for x in state], []
    for rnd in range(30):
        s = [(x + RC[12 * rnd + i]) % P for i, x in enumerate(s)]
        if rnd < 4 or rnd >= 26:
            if rnd:
                sbox += s
            s = [pow(x, 7, P) for x in s]
        else:
            sbox.append(s[0])
            s[0] = pow(s[0], 7, P)
        s = [sum(MDS[r][c] * s[c] for c in range(12)) % P for r in range(12)]
    return sbox, s


def swapped(inputs, sw):
    """(deltas, the state the permutation runs on) of a swap row"""
    d = [sw * (inputs[4 + i] - inputs[i]) % P for i in range(4)]
    return d, [(inputs[i] + d[i]) % P for i in range(4)] + [(inputs[4 + i] - d[i]) % P for i in range(4)] + list(inputs[8:12])


def reads(g):
    """(wires, constant columns) the generator reads on its row"""
    kind, p = g[0], g[3:8]
    if kind == ARITHMETIC:
        return [4 * k + j for k in range(p[0]) for j in range(3)], [p[1], p[2]]
    if kind == BASE_SPLIT:
        return [0], []
    if kind == CONSTANT:
        return [], [p[1] + l for l in range(p[0])]
    if kind == PUBLIC_INPUT:
        return [], []
    if kind == U32_MUL_ADD:
        return [p[1] * op + j for op in range(p[0]) for j in range(3)], []
    if kind == RANDOM_ACCESS:
        return [p[1] * cp + j for cp in range(p[0]) for j in [0] + list(range(2, 2 + (1 << p[2])))], []
    if kind == REDUCING:
        return list(range(4 + p[0])), []
    if kind == POSEIDON:
        return list(range(p[0], p[0] + 12)), []
    if kind == POSEIDON_SWAP:
        return list(range(p[0], p[0] + 12)) + [p[3]], []
    raise ValueError(kind)


def writes(g):
    """the wires the generator writes on its row, in the order compute() returns their values"""
    kind, p = g[0], g[3:8]
    if kind == ARITHMETIC:
        return [4 * k + 3 for k in range(p[0])]
    if kind == BASE_SPLIT:
        return [1 + l for l in range(p[0])]
    if kind == CONSTANT:
        return list(range(p[0]))
    if kind == PUBLIC_INPUT:
        return [0, 1, 2, 3]
    if kind == U32_MUL_ADD:
        return [p[1] * op + j for op in range(p[0]) for j in range(3, 5 + 2 * p[2])]
    if kind == RANDOM_ACCESS:
        return [p[1] * cp + j for cp in range(p[0]) for j in [1] + list(range(2 + (1 << p[2]), 2 + (1 << p[2]) + p[2]))]
    if kind == REDUCING:
        return list(range(4 + p[0], 4 + 3 * p[0]))
    if kind == POSEIDON:
        return list(range(p[2], p[2] + 106)) + list(range(p[1], p[1] + 12))
    if kind == POSEIDON_SWAP:
        return list(range(p[4], p[4] + 4)) + list(range(p[2], p[2] + 106)) + list(range(p[1], p[1] + 12))
    raise ValueError(kind)


def compute(g, w, k, pih):
    """the values of writes(g) from w, k = the values of reads(g)"""
    kind, p = g[0], g[3:8]
    if kind == ARITHMETIC:
        return [(k[0] * w[3 * i] * w[3 * i + 1] + k[1] * w[3 * i + 2]) % P for i in range(p[0])]
    if kind == BASE_SPLIT:                                   # limbs of the integer; bits above limbs * bits are dropped
        return [(w[0] >> (p[1] * l)) & ((1 << p[1]) - 1) for l in range(p[0])]
    if kind == CONSTANT:
        return list(k)
    if kind == PUBLIC_INPUT:
        return [int(x) for x in pih]
    if kind == U32_MUL_ADD:                                  # operands that are not u32 count with their low 32 bits
        out = []
        for op in range(p[0]):
            full = (w[3 * op] & M32) * (w[3 * op + 1] & M32) + (w[3 * op + 2] & M32)
            half = [full & M32, full >> 32]
            out += half + [(half[h] >> (2 * l)) & 3 for h in range(2) for l in range(p[2])]
        return out
    if kind == RANDOM_ACCESS:                                # the low `bits` bits of the index select
        out, ln = [], 1 << p[2]
        for cp in range(p[0]):
            c = w[(1 + ln) * cp:(1 + ln) * (cp + 1)]
            idx = c[0] & (ln - 1)
            out += [c[1 + idx]] + [(idx >> l) & 1 for l in range(p[2])]
        return out
    if kind == REDUCING:                                     # acc_i = acc_(i-1) alpha + c_i over F[X] / (X^2 - W)
        out, (al0, al1, a0, a1), W = [], w[:4], p[1]
        for l in range(p[0]):
            a0, a1 = (a0 * al0 + a1 * al1 * W + w[4 + l]) % P, (a0 * al1 + a1 * al0) % P
            out += [a0, a1]
        return out
    if kind == POSEIDON:
        sbox, out = permutation(w)
        return sbox + out
    if kind == POSEIDON_SWAP:
        d, st = swapped(w[:12], w[12])
        sbox, out = permutation(st)
        return d + sbox + out
    raise ValueError(kind)


_MEMO = {}


def _apply(out, written, consts, g, rows, pih):
    rows = rows[consts[g[1], rows] == np.uint64(g[2])]
    rw, rk = reads(g)
    ww = np.array(writes(g), dtype=np.int64)
    if not len(rows) or not len(ww):
        return
    keys = np.concatenate([out[rw][:, rows], consts[rk][:, rows]]).T.tolist()
    groups = {}
    for j, key in enumerate(keys):
        groups.setdefault(tuple(key), []).append(j)
    tag = (g[0],) + tuple(g[3:8]) + (tuple(pih) if g[0] == PUBLIC_INPUT else ())
    for key, js in groups.items():
        vals = _MEMO.get((tag, key))
        if vals is None:
            vals = _MEMO[(tag, key)] = np.array(compute(g, list(key[:len(rw)]), list(key[len(rw):]), pih), dtype=np.uint64)
        out[ww[:, None], rows[js][None, :]] = vals[:, None]
    written[ww[:, None], rows[None, :]] = True


def generate(wires, consts, gens, pih, sched=None):
    """(the table after witness generation, the mask of written cells): row-local (every generator on every row of its gate), or the
    replay of a level schedule"""
    out = np.ascontiguousarray(wires, dtype=np.uint64).copy()
    written = np.zeros(out.shape, dtype=bool)
    if sched is None:
        for g in gens:
            _apply(out, written, consts, g, np.arange(out.shape[1]), pih)
        return out, written
    flat, wflat = out.reshape(-1), written.reshape(-1)
    rows, lo, co = sched["rows"].astype(np.int64), sched["level_offsets"], sched["copy_offsets"]
    for lv in range(int(sched["n_levels"])):
        for g in gens:
            _apply(out, written, consts, g, rows[lo[lv]:lo[lv + 1]], pih)
        src, dst = sched["copy_src"][co[lv]:co[lv + 1]].astype(np.int64), sched["copy_dst"][co[lv]:co[lv + 1]].astype(np.int64)
        flat[dst] = flat[src]
        wflat[dst] = True
    return out, written


# ------------------------------------------------------------------------------------------------------------------------- the carry
def first_layer_carries(state):
    """per output r of the FIRST MDS layer of the permutation of `state`: does lo = al + (ah << 32) wrap (lo < al)?"""
    t = [pow((int(x) + RC[i]) % P, 7, P) for i, x in enumerate(state)]
    res = []
    for r in range(12):
        al = sum((t[c] & M32) * MDS[r][c] for c in range(12))
        ah = sum((t[c] >> 32) * MDS[r][c] for c in range(12))
        assert al < 1 << 64 and ah < 1 << 42
        res.append((al + (ah << 32)) % (1 << 64) < al)
    return res


_INV7 = pow(7, -1, P - 1)


def crafted_state(r, diagonal):
    """an input state whose first MDS layer carries in output r; the solved element is c = r (diagonal) or the next column with an odd
    coefficient"""
    rng = np.random.default_rng(1000 + 2 * r + diagonal)
    col = r if diagonal else next(c for c in range(r + 1, r + 13) if c % 12 != r and MDS[r][c % 12] % 2) % 12
    assert MDS[r][col] % 2
    while True:
        hi = [int(x) for x in rng.integers(0, M32, size=12)]                         # below 0xFFFFFFFF: the element stays canonical
        rest = sum(hi[c] * MDS[r][c] for c in range(12) if c != col)
        hi[col] = ((1 << 32) - 3 - rest) * pow(MDS[r][col], -1, 1 << 32) % (1 << 32)
        if hi[col] < M32:
            break
    target = [(h << 32) | M32 for h in hi]
    state = [(pow(t, _INV7, P) - RC[i]) % P for i, t in enumerate(target)]
    assert [pow((x + RC[i]) % P, 7, P) for i, x in enumerate(state)] == target and first_layer_carries(state)[r]
    return state


@functools.lru_cache(maxsize=None)
def poseidon_states():
    """[(name, state, designated carry output or None)]"""
    out = [("zero", [0] * 12, None), ("all p-1", [P - 1] * 12, None)]
    out += [("broadcast %#x" % v, [v] * 12, None) for v in MORE]
    out += [("unit %d" % i, [int(j == i) for j in range(12)], None) for i in range(12)]
    out += [("lattice", [MORE[j % 9] for j in range(12)], None)]
    for r in range(12):
        out += [("carry %d diag" % r, crafted_state(r, True), r), ("carry %d off" % r, crafted_state(r, False), r)]
    return out


# ------------------------------------------------------------------------------------------------------------------- building entries
def _rand_field(rng, shape):
    return np.ascontiguousarray(rng.integers(0, P, size=shape, dtype=np.uint64))


def one_level(n, reverse=True):
    """every row of the table in ONE level (in reversed order), no copies"""
    rows = np.arange(n, dtype=np.uint32)[::-1] if reverse else np.arange(n, dtype=np.uint32)
    return levels([rows], [[]])


def levels(level_rows, copies):
    """schedule dict from per-level row lists and per-level [(src cell, dst cell)]"""
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt) for x in xs]) if any(len(x) for x in xs) else np.zeros(0, dt)
    return {"n_levels": len(level_rows), "rows": np.ascontiguousarray(cat(level_rows, np.uint32)),
            "level_offsets": np.cumsum([0] + [len(r) for r in level_rows]).astype(np.uint32),
            "copy_src": cat([[s for s, _ in c] for c in copies], np.uint64), "copy_dst": cat([[d for _, d in c] for c in copies], np.uint64),
            "copy_offsets": np.cumsum([0] + [len(c) for c in copies]).astype(np.uint32)}


def _entry(name, log_n, num_wires, shapes, placed, seed, paths, pih=PIH_A, sched=None, crafted=(), dup=None, note=None):
    """shapes: [(kind, p0 .. p4)] -> generator k takes the rows of selector value k + 1; placed: [(row, shape index or None, {wire: value},
    {constant column: value})]; dup = (a, b, count): rows b .. b + count get the cells of rows a .. a + count"""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    gens = [(s[0], 0, k + 1) + tuple(s[1:]) + (0,) * (6 - len(s)) for k, s in enumerate(shapes)]
    w, k = _rand_field(rng, (num_wires, n)), _rand_field(rng, (NUM_CONSTANTS, n))
    k[0] = OTHER
    kind = np.zeros(n, dtype=np.int64)
    wr = [writes(g) for g in gens]
    for row, si, wd, kd in placed:
        if si is None:
            continue
        k[0, row], kind[row] = si + 1, gens[si][0]
        w[wr[si], row] = SENTINEL
        assert not set(wd) & set(wr[si]), (name, "an input cell is a generated cell")
        for j, v in wd.items():
            w[j, row] = v
        for j, v in kd.items():
            k[j, row] = v
    if sched is not None and len(sched["copy_dst"]):
        w.reshape(-1)[sched["copy_dst"].astype(np.int64)] = SENTINEL
    if dup:
        a, b, cnt = dup
        w[:, b:b + cnt], k[:, b:b + cnt], kind[b:b + cnt] = w[:, a:a + cnt], k[:, a:a + cnt], kind[a:a + cnt]
    assert int(w.max()) < P and int(k.max()) < P
    expected, written = generate(w, k, gens, pih, sched)
    return {"name": name, "log_n": log_n, "num_wires": num_wires, "num_constants": NUM_CONSTANTS, "wires": w, "consts": k, "pih": list(pih),
            "gens": gens, "sched": sched, "expected": expected, "written": written, "kind": kind, "paths": tuple(paths),
            "crafted": list(crafted), "note": note}


def _seq(groups, start=0):
    """[(shape, [(wires, consts)])] -> (shapes, placed) with the rows one after another"""
    shapes, placed, row = [], [], start
    for si, (shape, rows) in enumerate(groups):
        shapes.append(shape)
        for wd, kd in rows:
            placed.append((row, si, wd, kd))
            row += 1
    return shapes, placed


# --------------------------------------------------------------------------------------------------------------------- the short families
TRIPLES = list(itertools.product(EDGE, repeat=3))
PAIRS = list(itertools.product(EDGE, repeat=2))


def arithmetic_rows(n_ops):
    """every (c0, c1, a, b, c) over the lattice, 7776 rows: row t holds its tuple in op 0 and the triple (index + k) in op k, so every tuple
    also stands in every op of a 34-op row"""
    rows = []
    for (c0, c1), tri in itertools.product(PAIRS, range(216)):
        wd = {}
        for k in range(n_ops):
            wd[4 * k], wd[4 * k + 1], wd[4 * k + 2] = TRIPLES[(tri + k) % 216]
        rows.append((wd, {C0: c0, C1: c1}))
    return rows


def arithmetic(n_ops):
    shapes, placed = _seq([((ARITHMETIC, n_ops, C0, C1), arithmetic_rows(n_ops))])
    return _entry("arithmetic_%d" % n_ops, 13, 136, shapes, placed, 10 + n_ops, ("row_local", "coop", "coop_rows"))


BASE_SPLIT_SHAPES = [(1, 1), (1, 32), (2, 32), (64, 1), (63, 1), (32, 2), (16, 4), (21, 3), (32, 1)]     # (32, 1): tools/plonk_synth's


def base_split_values(limbs, bits):
    """the lattice, 2^k - 1 and 2^k at every limb boundary, values at and above 2^(limbs * bits)"""
    vals = list(MORE)
    for j in range(1, limbs + 1):
        vals += [(1 << (bits * j)) - 1, 1 << (bits * j), (1 << (bits * j)) + 1]
    top = limbs * bits
    vals += [(1 << top) | 5, (1 << 63) | (1 << top) | 1, P - 3]
    return sorted({v for v in vals if v < P})


def base_split_rows(limbs, bits):
    return [({0: v}, {}) for v in base_split_values(limbs, bits)]


def base_split():
    shapes, placed = _seq([((BASE_SPLIT, l, b), base_split_rows(l, b)) for l, b in BASE_SPLIT_SHAPES])
    return _entry("base_split", 13, 136, shapes, placed, 20, ("row_local", "coop", "coop_rows"))


CONSTANT_SHAPES = [(CONSTANT, 0, 1), (CONSTANT, 1, 7), (CONSTANT, 7, 1), (CONSTANT, 2, 3)]              # n = 0, 1, every constant column


def constant_rows():
    return [({}, {1 + c: MORE[(j + c) % 9] for c in range(7)}) for j in range(9)]


def constant_public_input(which):
    shapes, placed = _seq([(s, constant_rows()) for s in CONSTANT_SHAPES] + [((PUBLIC_INPUT,), [({}, {})] * 3)])
    return _entry("constant_public_input_%s" % which, 13, 136, shapes, placed, 30, ("row_local", "coop", "coop_rows"),
                  pih=PIH_A if which == "a" else PIH_B)


U32_VALUES = (0, 1, 1 << 16, 1 << 31, M32 - 1, M32)
U32_P_MINUS_1 = (M32, M32, M32)                             # (2^32 - 1)^2 + (2^32 - 1) = p - 1: high half 0xFFFFFFFF, low half 0
NOT_U32 = [(1 << 32, 1, 0), (P - 1, P - 1, P - 2), ((1 << 32) + 1, M32, P - (1 << 32)), (3, 1 << 32, 1 << 32), (1 << 63, 2, P - 1),
           (P - 2, (1 << 32) + 1, 1 << 32), (M32, P - 2, (1 << 63) | M32)]
U32_TRIPLES = list(itertools.product(U32_VALUES, repeat=3)) + NOT_U32
# (n_ops, stride, limbs per half): one op and the most the 136 wires take for 0, 1 and 16 limbs; 8 x 17 ends on wire 135; stride 45 leaves
# a gap of 8 cells behind every op; (3, 37, 16) is tools/plonk_synth's
U32_SHAPES = [(1, 5, 0), (27, 5, 0), (19, 7, 1), (1, 37, 16), (3, 37, 16), (8, 17, 6), (3, 45, 16)]


def u32_rows(n_ops, stride):
    rows = []
    for t in range(len(U32_TRIPLES)):
        wd = {}
        for op in range(n_ops):
            wd[stride * op], wd[stride * op + 1], wd[stride * op + 2] = U32_TRIPLES[(t + op) % len(U32_TRIPLES)]
        rows.append((wd, {}))
    return rows


def u32():
    shapes, placed = _seq([((U32_MUL_ADD, o, s, l), u32_rows(o, s)) for o, s, l in U32_SHAPES])
    return _entry("u32_mul_add", 13, 136, shapes, placed, 40, ("row_local", "coop", "coop_rows"))


# (copies, stride, bits): one copy and the most that fit for 1, 2 and 6 bits; 17 x 8 ends on wire 135; strides 11 and 80 leave gaps;
# (10, 8, 2) is tools/plonk_synth's
RA_SHAPES = [(1, 5, 1), (27, 5, 1), (17, 8, 2), (2, 11, 2), (10, 8, 2), (1, 72, 6), (1, 80, 6)]


def ra_indices(bits):
    ln = 1 << bits
    return [0, ln - 1, ln, ln + 1, M32, 1 << 32, (1 << 32) + 1, P - 1, (1 << 63) | (ln - 1), 1]


def ra_rows(copies, stride, bits, seed=0):
    """indices at and beyond the table's end, rotated over the copies, with items from the lattice (rotated per row and copy), then with
    random ones (all different: a wrong pick shows)"""
    rng = np.random.default_rng(600 + seed)
    ln, idx, rows = 1 << bits, ra_indices(bits), []
    for variant in range(2):
        for t in range(len(idx)):
            wd = {}
            for cp in range(copies):
                b = stride * cp
                wd[b] = idx[(t + cp) % len(idx)]
                for j in range(ln):
                    wd[b + 2 + j] = MORE[(j + t + cp) % 9] if variant == 0 else int(rng.integers(0, P, dtype=np.uint64))
            rows.append((wd, {}))
    for t in range(min(ln, 4)):                              # every index of the row inside the table: the rows the gate's constraints hold on
        wd = {}
        for cp in range(copies):
            wd[stride * cp] = (t + cp) % ln if t < 3 else ln - 1
            for j in range(ln):
                wd[stride * cp + 2 + j] = MORE[(j + 2 * t + cp) % 9]
        rows.append((wd, {}))
    return rows


def random_access():
    shapes, placed = _seq([((RANDOM_ACCESS, c, s, b), ra_rows(c, s, b, k)) for k, (c, s, b) in enumerate(RA_SHAPES)])
    return _entry("random_access", 13, 136, shapes, placed, 50, ("row_local", "coop", "coop_rows"))


# (K, W): K = 44 fills the 136 wires; (40, 7) is tools/plonk_synth's
REDUCING_SHAPES = [(44, 7), (44, 0), (44, 1), (44, M32), (1, 7), (1, M32), (40, 7)]


def reducing_rows(K, every=1):
    """alpha and the old accumulator over the lattice pairs (1296 rows), lattice coefficients"""
    rows = []
    for t, ((al0, al1), (a0, a1)) in enumerate(itertools.product(PAIRS, PAIRS)):
        if t % every == 0:
            wd = {0: al0, 1: al1, 2: a0, 3: a1}
            wd.update({4 + l: MORE[(t + l) % 9] for l in range(K)})
            rows.append((wd, {}))
    return rows


def reducing():
    shapes, placed = _seq([((REDUCING, K, W), reducing_rows(K, 6 if (K, W) == (40, 7) else 1)) for K, W in REDUCING_SHAPES])
    return _entry("reducing", 13, 136, shapes, placed, 60, ("row_local", "coop", "coop_rows"))


# ------------------------------------------------------------------------------------------------------------------ the Poseidon families
def plain_shape(lay):
    return (POSEIDON, lay["in_"], lay["out"], lay["sbox"])


def swap_shape(lay):
    return (POSEIDON_SWAP, lay["in_"], lay["out"], lay["sbox"], lay["swap"], lay["delta"])


def plain_rows(lay):
    """[(wires, consts, designated carry output or None)]"""
    return [({lay["in_"] + i: v for i, v in enumerate(st)}, {}, r) for _, st, r in poseidon_states()]


def swap_rows(lay):
    """every state that is not crafted under swap 0, 1, 2 and p - 1 (the broadcast ones have in[4+i] == in[i]; in the unit vectors and the
    two wrap states in[4+i] - in[i] wraps); every crafted state as the inputs under swap 0 and with its first two quarters exchanged under
    swap 1, so that the permutation runs on the crafted state both times"""
    rows = []

    def put(st, sw, r):
        wd = {lay["in_"] + i: v for i, v in enumerate(st)}
        wd[lay["swap"]] = sw
        rows.append((wd, {}, r))
    plain = [st for _, st, r in poseidon_states() if r is None]
    plain += [[P - 1] * 4 + [0] * 8, [0] * 4 + [P - 1] * 4 + [1] * 4]                  # 0 - (p - 1) and (p - 1) - 0
    for sw in (0, 1, 2, P - 1):
        for st in plain:
            put(st, sw, None)
    for _, st, r in poseidon_states():
        if r is not None:
            put(st, 0, r)
            put(st[4:8] + st[:4] + st[8:], 1, r)
    return rows


def _poseidon_entry(name, num_wires, shape, rows, seed, paths):
    placed = [(row, 0, wd, kd) for row, (wd, kd, _) in enumerate(rows)]
    crafted = [(row, r) for row, (_, _, r) in enumerate(rows) if r is not None]
    return _entry(name, 13, num_wires, [shape], placed, seed, paths, crafted=crafted)


def poseidon(which):
    nw, lay = PLAIN_LAYOUTS[which]
    return _poseidon_entry("poseidon_%s" % which, nw, plain_shape(lay), plain_rows(lay), 70, ("row_local", "coop", "coop_rows"))


def poseidon_swap(which):
    nw, lay = SWAP_LAYOUTS[which]
    return _poseidon_entry("poseidon_swap_%s" % which, nw, swap_shape(lay), swap_rows(lay), 80, ("row_local", "coop_rows"))


def state_of(entry, row):
    """the state the permutation of a Poseidon row of the entry runs on (after the swap), from the INPUT table"""
    g = entry["gens"][int(entry["consts"][0, row]) - 1]
    inp = [int(entry["wires"][g[3] + i, row]) for i in range(12)]
    return swapped(inp, int(entry["wires"][g[6], row]))[1] if g[0] == POSEIDON_SWAP else inp


# ------------------------------------------------------------------------------------------------------------------- levels and mixtures
def _short_groups(full):
    """(shape, rows) of the short families for the mixed tables; `full`: every family (else those tests/_merkle_reading.py reads too)"""
    g = [((BASE_SPLIT, 64, 1), base_split_rows(64, 1)), ((BASE_SPLIT, 2, 32), base_split_rows(2, 32)),
         ((RANDOM_ACCESS, 17, 8, 2), ra_rows(17, 8, 2, 20)), ((RANDOM_ACCESS, 1, 72, 6), ra_rows(1, 72, 6, 21)),
         ((CONSTANT, 7, 1), constant_rows()), ((PUBLIC_INPUT,), [({}, {})] * 2)]
    if full:
        g += [((ARITHMETIC, 34, C0, C1), arithmetic_rows(34)), ((U32_MUL_ADD, 3, 37, 16), u32_rows(3, 37)),
              ((U32_MUL_ADD, 8, 17, 6), u32_rows(8, 17)), ((REDUCING, 44, 7), reducing_rows(44))]
    return g


def _mixture(swap, full):
    """(shapes, short templates [(shape index, wires, consts)], Poseidon templates [(shape index, wires, consts, carry output)]): the short
    ones interleaved family by family; with `swap` two plain layouts and a swap one (170 wires), else upstream's plain one"""
    groups = _short_groups(full)
    shapes = [s for s, _ in groups]
    short, k = [], 0
    while any(k < len(rows) for _, rows in groups):
        short += [(si, rows[k][0], rows[k][1]) for si, (_, rows) in enumerate(groups) if k < len(rows)]
        k += 1
    pos_groups = [(plain_shape(PLAIN_LAYOUTS["upstream"][1]), plain_rows(PLAIN_LAYOUTS["upstream"][1]))]
    if swap:
        pos_groups += [(swap_shape(SWAP_LAYOUTS["last"][1]), swap_rows(SWAP_LAYOUTS["last"][1])),
                       (plain_shape(PLAIN_LAYOUTS["shifted"][1]), plain_rows(PLAIN_LAYOUTS["shifted"][1]))]
    pos, k = [], 0
    while any(k < len(rows) for _, rows in pos_groups):
        pos += [(len(shapes) + pi, rows[k][0], rows[k][1], rows[k][2]) for pi, (_, rows) in enumerate(pos_groups) if k < len(rows)]
        k += 1
    return shapes + [s for s, _ in pos_groups], short, pos


BOUNDARY_PATTERN = "PPPPSSSSSSSSPSOS"     # blocks of four rows: all Poseidon, short families only (twice), a mixture with a row of no gate


def boundary(swap):
    """log_n = 15: level 0 = rows 0 .. 16382 (16383 rows: sixteen lanes per row), level 1 = rows 16384 .. 32767 (16384 rows: one lane per
    row); row 16384 + j holds what row j holds, row 16383 is in no level and row 32767 = row 16383 is; every template of the mixture is
    in both levels, the arithmetic family's 7776 tuples among them"""
    shapes, short, pos = _mixture(swap, full=True)
    placed, crafted, ks, kp = [], [], 0, 0
    for row in range(16384):
        c = BOUNDARY_PATTERN[row % 16]
        if c == "S":
            placed.append((row,) + short[ks % len(short)])
            ks += 1
        elif c == "P":
            si, wd, kd, r = pos[kp % len(pos)]
            placed.append((row, si, wd, kd))
            if r is not None:
                crafted += [(row, r), (16384 + row, r)]
            kp += 1
    assert ks >= len(short) and kp >= len(pos)
    sched = levels([np.arange(16383), np.arange(16384, 32768)], [[], []])
    return _entry("boundary_%s" % ("swap" if swap else "plain"), 15, 170 if swap else 136, shapes, placed, 90, ("coop_rows" if swap else "coop",),
                  sched=sched, crafted=crafted, dup=(0, 16384, 16384))


THIN_LEVELS = ["P", "S", "PS", "SSS", "SPSSP", "SSSSP", "PP", "PSP", "SPPPS"]          # 1, 1, 2, 3, 5, 5, 2, 3, 5 rows


def thin_levels(swap):
    """levels of 1, 2, 3 and 5 rows at scattered rows: blocks of four with a Poseidon row and dead lanes, short rows only (the block leaves
    before the barriers), mixtures.  Copies carry the outputs of a crafted Poseidon row (level 0) and of later ones into Poseidon inputs
    and into the inputs of short rows of later levels."""
    n = 1 << 13
    shapes, short, pos = _mixture(swap, full=not swap)
    carry = [t for t in pos if t[3] is not None]
    rest = [t for t in pos if t[3] is None]
    placed, crafted, level_rows, p_rows, s_rows, ks, kp = [], [], [], [], [], 0, 0
    for lv, pat in enumerate(THIN_LEVELS):
        rows = []
        for c in pat:
            row = (len(placed) * 37 + 11) % n
            if c == "S":
                placed.append((row,) + short[(5 * ks) % len(short)])
                s_rows.append((lv, row, placed[-1][1]))
                ks += 1
            else:
                si, wd, kd, r = (carry if kp % 2 == 0 else rest)[(kp // 2) % (len(carry) if kp % 2 == 0 else len(rest))]
                placed.append((row, si, wd, kd))
                p_rows.append((lv, row, si))
                if r is not None:
                    crafted.append((row, r))
                kp += 1
            rows.append(row)
        level_rows.append(rows)
    gen = lambda si: shapes[si]
    copies = [[] for _ in THIN_LEVELS]
    fed = set()
    for a, (lv, row, si) in enumerate(p_rows):                 # Poseidon outputs 0 .. 3 -> the next Poseidon row of a LATER level, quarter a % 2
        for lv2, row2, si2 in p_rows[a + 1:]:
            if lv2 > lv and row2 not in fed:
                fed.add(row2)
                copies[lv] += [((gen(si)[2] + t) * n + row, (gen(si2)[1] + 4 * (a % 2) + t) * n + row2) for t in range(4)]
                break
        for lv2, row2, si2 in s_rows:                           # ... and output 4 -> the first input wire of one short row of a later level
            if lv2 > lv and row2 not in fed and gen(si2)[0] in (BASE_SPLIT, RANDOM_ACCESS):
                fed.add(row2)
                copies[lv].append(((gen(si)[2] + 4) * n + row, row2))
                break
    sched = levels(level_rows, copies)
    e = _entry("thin_levels_%s" % ("swap" if swap else "plain"), 13, 170 if swap else 136, shapes, placed, 95, ("coop_rows" if swap else "coop",),
               sched=sched, crafted=[c for c in crafted if c[0] not in fed])      # a row a copy feeds no longer holds its crafted state
    e["fed"] = sorted(fed)
    return e


# ------------------------------------------------------------------------------------------------------------------------ the catalogue
ENTRIES = [("arithmetic_1", lambda: arithmetic(1)), ("arithmetic_34", lambda: arithmetic(34)), ("base_split", base_split),
           ("constant_public_input_a", lambda: constant_public_input("a")), ("constant_public_input_b", lambda: constant_public_input("b")),
           ("u32_mul_add", u32), ("random_access", random_access), ("reducing", reducing),
           ("poseidon_upstream", lambda: poseidon("upstream")), ("poseidon_shifted", lambda: poseidon("shifted")),
           ("poseidon_last", lambda: poseidon("last")),
           ("poseidon_swap_upstream", lambda: poseidon_swap("upstream")), ("poseidon_swap_shifted", lambda: poseidon_swap("shifted")),
           ("poseidon_swap_last", lambda: poseidon_swap("last")),
           ("thin_levels_plain", lambda: thin_levels(False)), ("thin_levels_swap", lambda: thin_levels(True)),
           ("boundary_plain", lambda: boundary(False)), ("boundary_swap", lambda: boundary(True))]
NO_GRAPH_ENTRY = "thin_levels_plain"      # also run under SIPP_ROUTE_WITNESS_NO_GRAPH


@functools.lru_cache(maxsize=None)
def entry(name):
    e = dict(ENTRIES)[name]()
    assert e["name"] == name
    return e


def cases():
    """[(entry name, path)] without building an entry"""
    out = []
    for name, _ in ENTRIES:
        if name.startswith("poseidon_swap"):
            out += [(name, "row_local"), (name, "coop_rows")]
        elif name.startswith(("thin_levels", "boundary")):
            out.append((name, "coop_rows" if name.endswith("swap") else "coop"))
        else:
            out += [(name, "row_local"), (name, "coop"), (name, "coop_rows")]
    return out


def plan(e, path):
    """(generators, schedule or None) that send the entry through a launch path: row_local = sipp_plonk_generate_witness; coop = a
    schedule whose thin levels run plonk_witness_level_coop_kernel (at most one plain Poseidon generator in the list: one that no row
    holds is added where there is none); coop_rows = ... coop_rows_kernel (a swap generator in the list: one that no row holds is added
    where the list would not choose that kernel).  An entry without a schedule of its own gets one level of all its rows."""
    assert path in e["paths"], (e["name"], path)
    gens = list(e["gens"])
    if path == "row_local":
        return gens, None
    n_pos = sum(g[0] in (POSEIDON, POSEIDON_SWAP) for g in gens)
    per_row = n_pos > 1 or any(g[0] == POSEIDON_SWAP for g in gens)
    if path == "coop":
        assert not per_row
        if n_pos == 0:
            gens.append((POSEIDON, 0, OTHER - 2, 0, 12, 24, 0, 0))
    elif not per_row:
        gens.append((POSEIDON_SWAP, 0, OTHER - 1, 0, 12, 29, 24, 25))
    return gens, e["sched"] if e["sched"] is not None else one_level(1 << e["log_n"])


def kernels(gens, sched):
    """the kernels sipp_plonk_generate_witness_levels picks for the levels of a schedule (witness.hip, launch_all)"""
    n_pos = sum(g[0] in (POSEIDON, POSEIDON_SWAP) for g in gens)
    thin = "coop_rows" if n_pos > 1 or any(g[0] == POSEIDON_SWAP for g in gens) else "coop"
    counts = np.diff(sched["level_offsets"].astype(np.int64))
    return {"wide" if c >= COOP_BELOW_ROWS else thin for c in counts if c}


def first_mismatch(e, got, want=None):
    """None, or where the first differing cell lies: entry, wire, row, the row's family, both values, how many differ"""
    want = e["expected"] if want is None else want
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    j, r = int(bad[0][0]), int(bad[0][1])
    return "%s: wire %d row %d (%s, %s cell): got %#x, expected %#x; %d cells differ" % (
        e["name"], j, r, FAMILY[int(e["kind"][r])], "generated" if e["written"][j, r] else "untouched", int(got[j, r]), int(want[j, r]), len(bad))
