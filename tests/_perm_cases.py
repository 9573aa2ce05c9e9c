"""A catalogue of wire-permutation instances at the edges of the permutation argument (sipp_amd/csrc/plonk.hip: plonk_chunk_kernel,
plonk_scan_kernel, plonk_pp_kernel and the permutation terms of plonk_quotient_kernel), built explicitly rather than drawn at random.
CPU only: nothing here touches the GPU.  Used by tests/test_oracle_perm_edges.py (the catalogue against oracle/plonk.c, the second
reading in oracle/py/plonky2_generic.py and its own closed forms; proof that every edge class is reached), tests/test_gpu_perm_edges.py
(the device word for word against the catalogue).

Section A (ENTRIES_A, REFUSALS_A): Z and the partial products, sipp_plonk_zs_partial_products alone.  An entry function returns a dict:
name, log_n, R (routed wires), D (chunk size), C (challenges), wires [R][N] and sigmas [R][N] (uint64, as handed to the device), betas,
gammas (Python ints, as handed to the device), zs [C (1 + num_prods)][N] -- the expectation, from `zs_exact` below: Python integers,
every input reduced mod p first, one inversion per chunk cell with 1 / 0 = 0 -- tot [C][N] (the product of a row's chunks =
Z(g x) / Z(x)), closed (the name of the closed form the expectation must satisfy, see CLOSED_FORMS, or None), classes (the edge classes
the entry reaches), cells (the (challenge, column, row) cells where a factor vanishes) and reduced (True when some input is not
canonical: the device canonicalises, oracle/plonk.c expects canonical operands, so the oracle adapter must be given `oracle_inputs`).

Section B (ENTRIES_B, REFUSALS_B): quotient chunks and whole proofs at log_n 10 / 11 with a small FRI; the expectation is
oracle/plonk.c's.  An entry: name, log_n, R, D, C, rate_bits, wires, sigmas, kind ("proof": Z, quotient chunks with drawn challenges and
the whole proof; "quotient": the stand-alone quotient with the entry's own betas / gammas / alphas; "gate_terms": the quotient with
caller-supplied gate terms handed over as value + p), classes, and zero_quotient (every quotient coefficient is exactly 0)."""
import functools

import numpy as np

from tests import _oracle
from tests._gate_edges import EDGE_VALUES

P = _oracle.P
ROOT32 = 1753635133440165772            # a primitive 2^32-th root of unity
U64 = (1 << 64) - 1
FRI = dict(cap_height=1, nq=4, arity=4, fpb=3)
DIGEST = (17, 0, P - 1, 1 << 32)
E_BADARG, E_UNSUPPORTED = -1, -7
MAX_CHUNKS, MAX_CHALLENGES = 32, 8


def root_of_unity(log):
    return pow(ROOT32, 1 << (32 - log), P)


def powers(w, n):
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * w % P
    return out


def k_i(j):
    return pow(7, j, P)


def num_chunks(R, D):
    return -(-R // D)


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def identity_sigmas(log_n, R):
    """sigma_j(i) = 7^j w^i: every cell is its own cycle"""
    x = powers(root_of_unity(log_n), 1 << log_n)
    return _u64([[k_i(j) * xi % P for xi in x] for j in range(R)])


def sigmas_of(perm, log_n, R):
    """the sigma VALUES of a permutation of the positions (column j, row i) <-> index j N + i"""
    n = 1 << log_n
    x, k = powers(root_of_unity(log_n), n), [k_i(j) for j in range(R)]
    return _u64([k[t >> log_n] * x[t & (n - 1)] % P for t in perm.tolist()]).reshape(R, n)


def zs_exact(wires, sigmas, log_n, D, betas, gammas):
    """Z and the partial products over the integers mod p: columns Z_0 .. Z_(C-1), then per challenge its num_prods partial products;
    chunk q of a row is prod_j (w + beta 7^j x + gamma) / prod_j (w + beta sigma + gamma) over its wires, 0 when the denominator is 0.
    Returns (zs, tot): tot[c][i] = the product of row i's chunks."""
    n = 1 << log_n
    W, S = _obj(wires) % P, _obj(sigmas) % P
    R, m, C = W.shape[0], num_chunks(W.shape[0], D), len(betas)
    x = np.array(powers(root_of_unity(log_n), n), dtype=object)
    inv = np.frompyfunc(lambda d: pow(d, -1, P) if d else 0, 1, 1)
    zcols, pcols, tots = [], [], []
    for c in range(C):
        b, g = betas[c] % P, gammas[c] % P
        chunks = []
        for q in range(m):
            num = den = np.ones(n, dtype=object)
            for j in range(q * D, min((q + 1) * D, R)):
                num = num * ((W[j] + b * k_i(j) % P * x + g) % P) % P
                den = den * ((W[j] + b * S[j] + g) % P) % P
            chunks.append((num * inv(den) % P).tolist())
        z, zc, pc, tc = 1, [], [[] for _ in range(m - 1)], []
        for i in range(n):
            zc.append(z)
            acc, t = z, 1
            for q in range(m):
                acc, t = acc * chunks[q][i] % P, t * chunks[q][i] % P
                if q < m - 1:
                    pc[q].append(acc)
            tc.append(t)
            z = acc
        zcols.append(zc)
        pcols += pc
        tots.append(tc)
    return _u64(zcols + pcols), tots


def oracle_inputs(e):
    """what oracle/plonk.c must be given: every operand canonical"""
    return (_u64(_obj(e["wires"]) % P), _u64(_obj(e["sigmas"]) % P), [b % P for b in e["betas"]], [g % P for g in e["gammas"]])


def random_perm(rng, total, n_cycles=None, fixed=()):
    """a product of random cycles over every position but `fixed`; returns the permutation and a value per position, constant on cycles"""
    order = rng.permutation(total)
    order = order[~np.isin(order, list(fixed))] if len(fixed) else order
    n_cycles = n_cycles or max(1, total // 3)
    cuts = np.sort(rng.choice(np.arange(1, len(order)), size=min(n_cycles - 1, len(order) - 1), replace=False)) if len(order) > 1 else []
    perm, vals = np.arange(total), _oracle.rand_field(rng, (total,))
    start = 0
    for end in list(cuts) + [len(order)]:
        cyc = order[start:end]
        perm[cyc] = np.roll(cyc, -1)
        vals[cyc] = vals[cyc[0]]
        start = end
    return perm, vals


def _instance(seed, log_n, R, n_cycles=None, fixed=()):
    rng = np.random.default_rng(seed)
    perm, vals = random_perm(rng, R << log_n, n_cycles, fixed)
    return rng, vals.reshape(R, 1 << log_n).copy(), sigmas_of(perm, log_n, R), perm


def _challenges(rng, C):
    return [int(v) for v in _oracle.rand_field(rng, (C,))], [int(v) for v in _oracle.rand_field(rng, (C,))]


def _entry(name, log_n, D, wires, sigmas, betas, gammas, classes, closed=None, cells=(), reduced=False):
    zs, tot = zs_exact(wires, sigmas, log_n, D, betas, gammas)
    R = wires.shape[0]
    assert num_chunks(R, D) <= MAX_CHUNKS and len(betas) <= MAX_CHALLENGES and wires.shape == sigmas.shape == (R, 1 << log_n)
    return dict(name=name, log_n=log_n, R=R, D=D, C=len(betas), wires=np.ascontiguousarray(wires), sigmas=np.ascontiguousarray(sigmas),
                betas=list(betas), gammas=list(gammas), zs=zs, tot=tot, closed=closed, classes=set(classes), cells=list(cells), reduced=reduced)


# ------------------------------------------------------------------------------------------------------------ A1: shapes
# R, D, C and the classes the shape reaches
SHAPES = [
    (1, 2, 1, {"one_chunk"}),
    (8, 8, 2, {"one_chunk", "full_chunk"}),
    (9, 8, 2, {"ragged_one_wire"}),
    (63, 2, 1, {"chunks_32", "ragged_one_wire"}),
    (64, 2, 1, {"chunks_32", "full_chunk"}),
    (65, 64, 1, {"chunk_size_64", "ragged_one_wire"}),
    (5, 2, 8, {"challenges_8", "ragged_one_wire"}),
]
SHAPE_LOG_NS = (1, 5, 9, 12)            # 2 rows; one wave; fewer rows than the scan has threads; 4 rows per scan thread


def shape(log_n, R, D, C, classes):
    rng, wires, sigmas, _ = _instance(1000 + 100 * log_n + R, log_n, R)
    betas, gammas = _challenges(rng, C)
    cl = set(classes) | {"log_n_%d" % log_n} | ({"chunk_size_16_to_64"} if D >= 16 else set())
    return _entry("shape_n%d_R%d_D%d_C%d" % (log_n, R, D, C), log_n, D, wires, sigmas, betas, gammas, cl)


# name, log_n, R, D, C, the exact code: refused by check() before any kernel runs
REFUSALS_A = [
    ("chunks_33", 5, 65, 2, 1, E_UNSUPPORTED),
    ("challenges_9", 5, 4, 2, 9, E_UNSUPPORTED),
    ("chunk_size_3", 5, 4, 3, 1, E_UNSUPPORTED),
    ("chunk_size_1", 5, 4, 1, 1, E_UNSUPPORTED),
    ("chunk_size_128", 5, 4, 128, 1, E_UNSUPPORTED),
    ("log_n_0", 0, 4, 2, 1, E_BADARG),
    ("log_n_25", 25, 4, 2, 1, E_BADARG),
]

# ------------------------------------------------------------------------------------------------------------ A2: closed forms
LOG_N, R13, D4 = 5, 13, 4               # 4 chunks, the last one a single wire


def identity():
    rng = np.random.default_rng(21)
    n = 1 << LOG_N
    betas, gammas = _challenges(rng, 2)
    return _entry("identity", LOG_N, D4, _oracle.rand_field(rng, (R13, n)), identity_sigmas(LOG_N, R13), betas, gammas, {"closed_form"}, "all_one")


def beta_zero():
    rng, _, sigmas, _ = _instance(22, LOG_N, R13)
    _, gammas = _challenges(rng, 2)
    return _entry("beta_zero", LOG_N, D4, _oracle.rand_field(rng, (R13, 1 << LOG_N)), sigmas, [0, 0], gammas, {"closed_form", "beta_0"}, "all_one")


def constant_wires(k):
    rng, wires, sigmas, _ = _instance(30 + k, LOG_N, R13)
    betas, gammas = _challenges(rng, 2)
    wires[:] = EDGE_VALUES[k]
    return _entry("constant_wires_%d" % k, LOG_N, D4, wires, sigmas, betas, gammas, {"closed_form", "edge_wires"}, "closure")


def one_cycle():
    rng, wires, sigmas, perm = _instance(40, LOG_N, R13, n_cycles=1)
    seen, t = 0, 0
    while True:                           # really ONE cycle through all R N cells
        t, seen = int(perm[t]), seen + 1
        if t == 0:
            break
    assert seen == R13 << LOG_N and len(set(wires.reshape(-1).tolist())) == 1
    betas, gammas = _challenges(rng, 2)
    return _entry("one_cycle", LOG_N, D4, wires, sigmas, betas, gammas, {"closed_form", "one_cycle"}, "closure")


TRANSPOSITION = ((1, 3), (9, 20))        # (column, row): chunk 0 and chunk 2, rows 3 and 20


def transposition():
    rng = np.random.default_rng(41)
    n = 1 << LOG_N
    (ja, ia), (jb, ib) = TRANSPOSITION
    perm = np.arange(R13 * n)
    perm[ja * n + ia], perm[jb * n + ib] = jb * n + ib, ja * n + ia
    wires = _oracle.rand_field(rng, (R13, n))
    wires[jb, ib] = wires[ja, ia]
    betas, gammas = _challenges(rng, 2)
    return _entry("transposition", LOG_N, D4, wires, sigmas_of(perm, LOG_N, R13), betas, gammas, {"closed_form", "transposition"}, "transposition")


def _closure(e):
    for c in range(e["C"]):
        prod = 1
        for t in e["tot"][c]:
            prod = prod * t % P
        if prod != 1 or int(e["zs"][c, 0]) != 1:
            return False
    return True


def _transposition_form(e):
    (_, ia), (_, ib) = TRANSPOSITION
    z = e["zs"][:e["C"]]
    return _closure(e) and (z[:, :ia + 1] == 1).all() and (z[:, ib + 1:] == 1).all() and (z[:, ia + 1:ib + 1] != 1).all()


CLOSED_FORMS = {
    "all_one": lambda e: bool((e["zs"] == 1).all()),
    "closure": _closure,                 # every copy constraint holds: the rows' products multiply to 1 and Z(w^0) = 1
    "transposition": _transposition_form,   # Z leaves 1 behind the first swapped cell's row and returns to it behind the second's
}

# ------------------------------------------------------------------------------------------------------------ A3: vanishing denominator
SPECIAL = 1                              # the challenge (of 3) whose gamma is chosen; the others stay random


def _neg(v):
    return (-v) % P


def vanishing_denominator(name, cols, row, log_n=LOG_N, zero_over_zero=False):
    """gamma_SPECIAL = -(w + beta sigma) at (cols[0], row); a second column of the same row gets the wire that makes its factor vanish
    too; zero_over_zero: sigma fixes the cell, so the numerator's factor is the same 0"""
    n = 1 << log_n
    fixed = [cols[0] * n + row] if zero_over_zero else ()
    j0, seed = cols[0], 50 + len(name) + cols[0]
    while True:                           # sigma fixes the cell exactly when the entry asks for 0 / 0
        rng, wires, sigmas, perm = _instance(seed, log_n, R13, fixed=fixed)
        if [int(perm[j * n + row]) == j * n + row for j in cols] == [zero_over_zero] + [False] * (len(cols) - 1):
            break
        seed += 1000
    betas, gammas = _challenges(rng, 3)
    b = betas[SPECIAL]
    # a wire of its own: with the cycle's value, the NUMERATOR of the cell sigma points to (the same wire) would vanish with this denominator
    wires[j0, row] = _oracle.rand_field(rng, (1,))[0]
    gammas[SPECIAL] = _neg(int(wires[j0, row]) + b * int(sigmas[j0, row]))
    for j in cols[1:]:
        wires[j, row] = _neg(gammas[SPECIAL] + b * int(sigmas[j, row]))
    cl = {"vanishing_denominator", "den_chunk_%d" % (j0 // D4)} | ({"den_two_chunks"} if len(cols) > 1 else set()) | \
        ({"zero_over_zero"} if zero_over_zero else set()) | ({"den_ragged_last"} if j0 == R13 - 1 else set())
    return _entry(name, log_n, D4, wires, sigmas, betas, gammas, cl, cells=[(SPECIAL, j, row) for j in cols])


# ------------------------------------------------------------------------------------------------------------ A4: vanishing numerator
def vanishing_numerator(name, log_n, rows, col=6):
    """gamma_0 = -(w + beta 7^col w^row) for the first row; a further row gets the wire that makes its factor vanish under the same gamma"""
    n = 1 << log_n
    seed = 70 + log_n + rows[0]
    while True:                           # sigma moves the cells: their denominators do not vanish with the numerators
        rng, wires, sigmas, perm = _instance(seed, log_n, R13)
        if all(int(perm[col * n + r]) != col * n + r for r in rows):
            break
        seed += 1000
    betas, gammas = _challenges(rng, 2)
    x, b = powers(root_of_unity(log_n), n), betas[0]
    # a wire of its own: with the cycle's value, the DENOMINATOR of the cell that sigma sends here (the same wire) would vanish too
    wires[col, rows[0]] = _oracle.rand_field(rng, (1,))[0]
    gammas[0] = _neg(int(wires[col, rows[0]]) + b * k_i(col) % P * x[rows[0]])
    for r in rows[1:]:
        wires[col, r] = _neg(gammas[0] + b * k_i(col) % P * x[r])
    cl = {"vanishing_numerator"} | {"num_row_%s" % ("last" if r == n - 1 else r) for r in rows} | {"log_n_%d" % log_n}
    return _entry(name, log_n, D4, wires, sigmas, betas, gammas, cl, cells=[(0, col, r) for r in rows])


# ------------------------------------------------------------------------------------------------------------ A5: operand edges
def edge_wires():
    rng, _, sigmas, _ = _instance(90, LOG_N, R13)
    betas, gammas = _challenges(rng, 2)
    wires = _u64(EDGE_VALUES)[rng.integers(0, len(EDGE_VALUES), size=(R13, 1 << LOG_N))]
    return _entry("edge_wires", LOG_N, D4, wires, sigmas, betas, gammas, {"edge_wires"})


EDGE_CHALLENGES = (0, 1, P - 1, P, P + 1, U64)


def edge_challenges():
    """beta and gamma through 0, 1, p - 1 and the non-canonical p, p + 1, 2^64 - 1, every beta against another gamma.  The device
    canonicalises them; the oracle adapter must be given the reduced values (reduced=True)."""
    rng, wires, sigmas, _ = _instance(91, LOG_N, R13)
    return _entry("edge_challenges", LOG_N, D4, wires, sigmas, list(EDGE_CHALLENGES), list(EDGE_CHALLENGES[2:] + EDGE_CHALLENGES[:2]),
                  {"edge_challenges", "noncanonical_challenges", "beta_0"}, reduced=True)


def noncanonical_wires():
    """every third wire cell handed over as value + p (values below 2^32 - 1, so that the sum fits 64 bits; 2^64 - 1 among them): the
    expectation is that of the reduced values, reduced=True"""
    rng, wires, sigmas, _ = _instance(92, LOG_N, R13)
    betas, gammas = _challenges(rng, 2)
    small = rng.integers(0, (1 << 32) - 1, size=wires.shape, dtype=np.uint64)
    small[0, 0], small[12, 30] = 0, (1 << 32) - 2
    a, r = np.indices(wires.shape)
    wires = np.where((a + r) % 3 == 0, small + np.uint64(P), wires)
    return _entry("noncanonical_wires", LOG_N, D4, wires, sigmas, betas, gammas, {"noncanonical_wires"}, reduced=True)


def _named(f, *a, **k):
    g = functools.lru_cache(maxsize=None)(functools.partial(f, *a, **k))
    return g


ENTRIES_A = [("shape_n%d_R%d_D%d_C%d" % (ln, R, D, C), _named(shape, ln, R, D, C, frozenset(cl))) for ln in SHAPE_LOG_NS for R, D, C, cl in SHAPES]
ENTRIES_A += [
    ("identity", _named(identity)),
    ("beta_zero", _named(beta_zero)),
] + [("constant_wires_%d" % k, _named(constant_wires, k)) for k in range(len(EDGE_VALUES))] + [
    ("one_cycle", _named(one_cycle)),
    ("transposition", _named(transposition)),
    # (a zero in chunk 0 makes every partial product of its row 0 in any reading: den_chunk_0 pins the value, the entries behind it are
    # the ones that tell "this chunk" from "the whole row")
    ("den_chunk_0", _named(vanishing_denominator, "den_chunk_0", (1,), 7)),
    ("den_chunk_2", _named(vanishing_denominator, "den_chunk_2", (9,), 7)),
    ("den_ragged_last", _named(vanishing_denominator, "den_ragged_last", (12,), 30)),
    ("den_two_chunks", _named(vanishing_denominator, "den_two_chunks", (5, 10), 0)),
    ("den_zero_over_zero", _named(vanishing_denominator, "den_zero_over_zero", (6,), 19, zero_over_zero=True)),
    ("den_chunk_2_n12", _named(vanishing_denominator, "den_chunk_2_n12", (9,), 3001, log_n=12)),
    ("num_row_0", _named(vanishing_numerator, "num_row_0", LOG_N, (0,))),
    ("num_row_last", _named(vanishing_numerator, "num_row_last", LOG_N, ((1 << LOG_N) - 1,))),
    ("num_rows_3_4_n12", _named(vanishing_numerator, "num_rows_3_4_n12", 12, (3, 4))),
    ("num_row_3_n12", _named(vanishing_numerator, "num_row_3_n12", 12, (3,))),
    ("num_row_4_n12", _named(vanishing_numerator, "num_row_4_n12", 12, (4,))),
    ("num_row_1023_n10", _named(vanishing_numerator, "num_row_1023_n10", 10, (1023,))),
    ("edge_wires", _named(edge_wires)),
    ("edge_challenges", _named(edge_challenges)),
    ("noncanonical_wires", _named(noncanonical_wires)),
]
IDS_A = [name for name, _ in ENTRIES_A]


def first_mismatch(got, want):
    """(column, row) of the first differing cell and how many differ, or None"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else "first mismatching (column, row): (%d, %d), %d cells differ" % (bad[0][0], bad[0][1], len(bad))


# ------------------------------------------------------------------------------------------------------------ section B
def fri_params(e):
    return _oracle.fri_params(rate_bits=e["rate_bits"], cap_height=FRI["cap_height"], pow_bits=6, num_queries=FRI["nq"], pow_rule=0, hiding=0,
                              arity_bits=FRI["arity"], final_poly_bits=FRI["fpb"], degree_bits=e["log_n"])


def _b(name, log_n, R, D, C, rate_bits, wires, sigmas, kind, classes, **kw):
    cl = set(classes) | ({"rate_above_chunk"} if (1 << rate_bits) > D else set()) | ({"log_n_11"} if log_n == 11 else set())
    return dict(name=name, log_n=log_n, R=R, D=D, C=C, rate_bits=rate_bits, wires=wires, sigmas=sigmas, kind=kind, classes=cl,
                zero_quotient=kw.pop("zero_quotient", False), **kw)


def proof_config(log_n, R, D, C, rate_bits, classes=frozenset()):
    _, wires, sigmas, _ = _instance(2000 + log_n + R + rate_bits, log_n, R)
    return _b("proof_n%d_R%d_D%d_C%d_r%d" % (log_n, R, D, C, rate_bits), log_n, R, D, C, rate_bits, wires, sigmas, "proof", classes)


def proof_identity():
    rng = np.random.default_rng(2100)
    return _b("proof_identity", 10, R13, D4, 2, 3, _oracle.rand_field(rng, (R13, 1 << 10)), identity_sigmas(10, R13), "proof", {"identity"},
              zero_quotient=True)


def proof_constant_wires():
    _, wires, sigmas, _ = _instance(2101, 10, R13)
    wires[:] = P - 1
    return _b("proof_wires_p_minus_1", 10, R13, D4, 2, 3, wires, sigmas, "proof", {"edge_wires"})


QUOTIENT_CHALLENGES = {                  # betas, gammas, alphas
    "alpha_0": ([3, 5], [7, 11], [0, 0]),                                    # only L_0 (Z - 1) survives
    "alpha_1": ([P - 3, 1 << 32], [(1 << 32) - 1, P - 1], [1, 1]),
    "noncanonical": ([P + 5, U64], [P, P + 1], [U64, P + 2]),
}


def quotient_alone(which):
    _, wires, sigmas, _ = _instance(2200, 10, R13)
    betas, gammas, alphas = QUOTIENT_CHALLENGES[which]
    return _b("quotient_" + which, 10, R13, D4, 2, 3, wires, sigmas, "quotient", {"quotient_" + which}, betas=list(betas), gammas=list(gammas),
              alphas=list(alphas), reduced=which == "noncanonical")


GATE_TERM_DEFECT = (1 << 32) - 2          # value + p = 2^64 - 1


def quotient_gate_terms():
    """the product gates of oracle/plonk.h's synthetic circuit (term k = w_3k w_3k+1 - w_3k+2 on the quotient coset), every term cell
    below 2^32 - 1 handed to the device as value + p.  The terms of a random satisfied gate are uniform there and never that small, so
    gates 0 and 1 have CONSTANT columns: gate 0 holds (its term is 0 on the whole coset, handed over as p), gate 1 misses by
    GATE_TERM_DEFECT (its term is that constant, handed over as 2^64 - 1); gate 2 is an ordinary satisfied gate.  The quotient of a
    witness that misses a gate is no polynomial of the usual degree, but its chunks are the same arithmetic on both sides."""
    K = 3
    wires, sigmas, _ = _oracle.plonk_gate_instance(2300, 10, 9, K)
    rng = np.random.default_rng(2301)
    for k, defect in ((0, 0), (1, GATE_TERM_DEFECT)):
        a, b = (int(v) for v in _oracle.rand_field(rng, (2,)))
        wires[3 * k], wires[3 * k + 1], wires[3 * k + 2] = a, b, (a * b - defect) % P
    betas, gammas = _challenges(rng, 1)
    return _b("quotient_gate_terms_plus_p", 10, 9, 2, 1, 2, wires, sigmas, "gate_terms", {"noncanonical_gate_terms"}, betas=betas, gammas=gammas,
              alphas=[int(_oracle.rand_field(rng, (1,))[0])], num_mul=K, reduced=True)


def lift(values):
    """value + p wherever that fits in 64 bits"""
    v = np.asarray(values, dtype=np.uint64)
    return np.where(v < np.uint64((1 << 32) - 1), v + np.uint64(P), v)


PROOF_CONFIGS = [
    (10, 9, 2, 1, 3, ()), (10, 13, 4, 2, 3, ()), (10, 9, 2, 1, 2, ()), (11, 13, 4, 2, 3, ()),
    (10, 63, 2, 1, 1, ("chunks_32",)), (10, 5, 2, 8, 1, ("challenges_8",)), (10, 1, 2, 1, 1, ("one_chunk",)), (10, 8, 8, 2, 3, ("one_chunk",)),
]
ENTRIES_B = [("proof_n%d_R%d_D%d_C%d_r%d" % c[:5], _named(proof_config, *c[:5], frozenset(c[5]))) for c in PROOF_CONFIGS] + [
    ("proof_identity", _named(proof_identity)),
    ("proof_wires_p_minus_1", _named(proof_constant_wires)),
] + [("quotient_" + w, _named(quotient_alone, w)) for w in QUOTIENT_CHALLENGES] + [
    ("quotient_gate_terms_plus_p", _named(quotient_gate_terms)),
]
IDS_B = [name for name, _ in ENTRIES_B]

# name, R, D, C, rate_bits, gate terms (count, pointer given), the exact code; all at log_n 10
REFUSALS_B = [
    ("chunk_size_16_rate_3", 16, 16, 1, 3, (0, False), E_UNSUPPORTED),      # sipp_plonk_zs_partial_products takes this chunk size
    ("rate_bits_4", 8, 8, 1, 4, (0, False), E_UNSUPPORTED),
    ("gate_terms_null", 9, 2, 1, 1, (3, False), E_BADARG),
]


def bitrev_order(log):
    return np.array([int(format(j, "0%db" % log)[::-1], 2) for j in range(1 << log)])
