"""The case table of the generic opening proofs (sipp_commit_batch_ex + sipp_fri_prove_openings) at the edges of their documented
range, with the builders that turn a case into CPU-oracle batches.  CPU only: nothing here touches the GPU.  Used by
tests/test_oracle_fri_edges.py (the table against both verifiers and the Python reading), tests/test_gpu_fri_edges.py (the device
proofs word for word against the oracle's) and scripts/stress_fri.py (the random configuration generator, `stress_config`).

A case names: log_n / rate_bits / cap_height; the oracles (widths, which are salted, which are handed over as values and which as
coefficients); a column generator (`random`, `structured`, `zero`); the batches; the FRI parameters; the transcript in front of the
proof (observations, then `gets` challenges drawn, so that the challenger arrives with pending output)."""
import ctypes as C

import numpy as np

from tests import _oracle

P = _oracle.P
ROOT32 = 1753635133440165772            # a primitive 2^32-th root of unity (the oracle's, gl.h)


def root_of_unity(log):
    return pow(ROOT32, 1 << (32 - log), P)


def scale(pt, s):
    """the extension element pt times the base-field element s"""
    return (pt[0] * s % P, pt[1] * s % P)


def all_columns(widths):
    return [(k, 0, w) for k, w in enumerate(widths)]


def sub_columns(widths):
    """a sub-range of oracle 0 and all of the last oracle (like zs / next-row openings); never an empty batch"""
    w0 = widths[0]
    sub = [(0, 1 if w0 >= 2 else 0, w0 - 1 if w0 >= 3 else w0)]
    if len(widths) > 1:
        sub.append((len(widths) - 1, 0, widths[-1]))
    return sub


class Case:
    def __init__(self, id, log_n=10, rate_bits=1, cap_height=4, widths=(3, 2), salted=None, from_values=None, columns="random",
                 seed=0, point=None, batches=None, fri=None, prefix=(7, 7, 7), gets=0, stress_seed=None):
        self.id, self.log_n, self.rate_bits, self.cap_height = id, log_n, rate_bits, cap_height
        self.widths = tuple(widths)
        self.salted = tuple(salted) if salted is not None else (False,) * len(self.widths)
        # oracle 0 from values, the others from coefficients (as tests/test_oracle_fri_generic.random_instance hands them over)
        self.from_values = tuple(from_values) if from_values is not None else tuple(k == 0 for k in range(len(self.widths)))
        self.columns, self.seed, self.point, self.batches = columns, seed, point, batches
        # FRI parameters: arity 16, final polynomial of 2^5 coefficients, 5 queries, 6 proof-of-work bits unless the case says otherwise
        self.fri = dict(pow_bits=6, num_queries=5, pow_rule=0, arity_bits=4, final_poly_bits=5)
        self.fri.update(fri or {})
        self.prefix, self.gets, self.stress_seed = tuple(prefix), gets, stress_seed

    def __repr__(self):
        return self.id


class Instance:
    """a built case: the oracle's batches, the batches [(point, ranges)], the oracle-side FriParams"""

    def __init__(self, case, oracles, batches, fp, log_n):
        self.case, self.oracles, self.batches, self.fp, self.log_n = case, oracles, batches, fp, log_n
        self.caps = [o.cap for o in oracles]
        self.ncols = [o.ncols for o in oracles]
        self.n_salt = [o.n_salt for o in oracles]

    def verifier_args(self):
        return (self.caps, self.ncols, self.n_salt, self.batches, self.log_n, self.fp)

    def witness_index(self):
        """the position of the proof-of-work witness in the flat proof: header, opened values, commit caps, final polynomial"""
        k = sum(e - b for _, ranges in self.batches for _, b, e in ranges)
        arities = [self.fp.arity_bits[i] for i in range(self.fp.n_rounds)]
        return 8 + 2 * k + len(arities) * (4 << self.fp.cap_height) + 2 * ((1 << self.log_n) >> sum(arities))


def structured_coefficients(rng, ncols, n):
    """coefficient column c cycles through: all 0, the constant p - 1, X^(n-1) alone, every coefficient p - 1, words whose halves are
    all ones (2^32 - 1 and p - 1 = 0xFFFFFFFF00000000, alternating), random"""
    cols = np.zeros((ncols, n), dtype=np.uint64)
    for c in range(ncols):
        k = c % 6
        if k == 1:
            cols[c, 0] = P - 1
        elif k == 2:
            cols[c, n - 1] = 1
        elif k == 3:
            cols[c] = P - 1
        elif k == 4:
            cols[c, 0::2], cols[c, 1::2] = 0xFFFFFFFF, 0xFFFFFFFF00000000
        elif k == 5:
            cols[c] = _oracle.rand_field(rng, n)
    return cols


def values_of(coeffs, log_n):
    """the values on the trace subgroup of coefficient columns (what PolynomialBatch::from_values is handed)"""
    vals = np.ascontiguousarray(coeffs, dtype=np.uint64).copy()
    L = _oracle.load()
    for c in range(vals.shape[0]):
        L.orc_fft(vals[c], log_n)
    return vals


def fri_params(case):
    kw = dict(case.fri)
    if "arities" not in kw:
        kw["degree_bits"] = case.log_n
    return _oracle.fri_params(rate_bits=case.rate_bits, cap_height=case.cap_height, hiding=1, **kw)


def challenger(case):
    """a fresh oracle challenger with the case's transcript in front: its observations, then `gets` challenges drawn"""
    if case.stress_seed is not None:
        return _oracle.challenger([case.stress_seed, 1, 2])
    ch = _oracle.challenger(case.prefix)
    L = _oracle.load()
    L.orc_chal_get.restype = C.c_uint64
    L.orc_chal_get.argtypes = [C.POINTER(_oracle.OrcChallenger)]
    for _ in range(case.gets):
        L.orc_chal_get(C.byref(ch))
    return ch


def build(case):
    if case.stress_seed is not None:
        cfg, rng = stress_config(case.stress_seed)
        oracles, batches = stress_data(cfg, rng)
        return Instance(case, oracles, batches, cfg["fp"], cfg["log_n"])
    rng = np.random.default_rng(case.seed)
    log_n, n, m = case.log_n, 1 << case.log_n, 1 << (case.log_n + case.rate_bits)
    oracles = []
    for k, w in enumerate(case.widths):
        if case.columns == "random":
            data = _oracle.rand_field(rng, (w, n))
        else:
            data = structured_coefficients(rng, w, n) if case.columns == "structured" else np.zeros((w, n), dtype=np.uint64)
            if case.from_values[k]:
                data = values_of(data, log_n)
        salt = _oracle.rand_field(rng, (4, m)) if case.salted[k] else None
        oracles.append(_oracle.SaltedBatch(data, log_n, case.rate_bits, case.cap_height, from_values=case.from_values[k], salt=salt))
    zeta = tuple(int(x) for x in _oracle.rand_field(rng, 2))
    g = root_of_unity(log_n)
    if case.batches is not None:
        batches = case.batches(zeta, g)
    else:
        z = case.point if case.point is not None else zeta
        batches = [(z, all_columns(case.widths)), (scale(z, g), sub_columns(case.widths))]
    return Instance(case, oracles, batches, fri_params(case), log_n)


def device_inputs(inst):
    """per oracle (data, from_coeffs, salt) as sipp_commit_batch_ex takes them: the oracle's own coefficients, or the values
    re-derived from them, by the case's hand-over"""
    out = []
    fv = inst.case.from_values if inst.case.stress_seed is None else [k % 2 == 0 for k in range(len(inst.oracles))]
    for k, o in enumerate(inst.oracles):
        coeffs = o.coeffs
        out.append((values_of(coeffs, inst.log_n), False, o.salt) if fv[k] else (coeffs, True, o.salt))
    return out


# ---- the random configurations of scripts/stress_fri.py, as a function of the seed --------------------------------------------------
def stress_config(seed):
    """random FriParams (blowup 2 / 4 / 8, cap heights, constant or mixed arities 2 .. 16, final polynomial sizes, both proof-of-work
    rules, query counts), a random number of oracles with random widths and salting.  Returns (cfg, rng): the generator goes on into
    stress_data, which draws the columns, the point and the second batch from it."""
    rng = np.random.default_rng(seed)
    log_n = int(rng.integers(10, 15))       # the GPU layer supports degree bits 10 .. 24
    rate_bits = int(rng.integers(1, 4))
    n_or = int(rng.integers(1, 5))
    widths = [int([1, 2, 4, 5, 8, 9, 17, 33][int(rng.integers(0, 8))]) for _ in range(n_or)]
    salted = [bool(rng.integers(0, 2)) for _ in range(n_or)]
    mixed = bool(rng.integers(0, 3) == 0)
    pow_rule = int(rng.integers(0, 2))
    nq = int(rng.integers(1, 13))
    pow_bits = int(rng.integers(0, 11))
    if mixed:
        arities, left = [], log_n
        while left > 0 and len(arities) < 6 and rng.integers(0, 4):
            a = int(rng.integers(1, min(4, left) + 1))
            arities.append(a)
            left -= a
        if not arities:
            arities = [min(2, log_n)]
        final_bits = log_n - sum(arities)
        cap_height = int(rng.integers(0, min(5, final_bits + rate_bits) + 1))
        fp = _oracle.fri_params(rate_bits=rate_bits, cap_height=cap_height, pow_bits=pow_bits, num_queries=nq, pow_rule=pow_rule, hiding=1,
                                arities=arities)
        desc = "arities %s" % arities
    else:
        arity = int(rng.integers(1, 5))
        final_poly_bits = int(rng.integers(0, 6))
        cap_height = int(rng.integers(0, 6))
        fp = _oracle.fri_params(rate_bits=rate_bits, cap_height=cap_height, pow_bits=pow_bits, num_queries=nq, pow_rule=pow_rule, hiding=1,
                                arity_bits=arity, final_poly_bits=final_poly_bits, degree_bits=log_n)
        desc = "arity %d final %d rounds %d" % (arity, final_poly_bits, fp.n_rounds)
    tag = "seed %d: log_n %d blowup %d cap %d %s pow %d/%d q %d widths %s salted %s" % (
        seed, log_n, 1 << rate_bits, cap_height, desc, pow_bits, pow_rule, nq, widths, [int(x) for x in salted])
    cfg = dict(seed=seed, log_n=log_n, rate_bits=rate_bits, cap_height=cap_height, widths=widths, salted=salted, mixed=mixed, fp=fp, tag=tag)
    return cfg, rng


def stress_data(cfg, rng):
    """the oracles (even ones from values, odd ones from coefficients) and the batches of a stress configuration: everything at zeta,
    then random sub-ranges at g zeta.  Raises where the oracle itself refuses the shape."""
    log_n, rate_bits, widths = cfg["log_n"], cfg["rate_bits"], cfg["widths"]
    n, m, n_or = 1 << log_n, 1 << (log_n + rate_bits), len(widths)
    oracles = []
    for k in range(n_or):
        vals = _oracle.rand_field(rng, (widths[k], n))
        salt = _oracle.rand_field(rng, (4, m)) if cfg["salted"][k] else None
        oracles.append(_oracle.SaltedBatch(vals, log_n, rate_bits, cfg["cap_height"], from_values=(k % 2 == 0), salt=salt))
    zeta = tuple(int(x) for x in _oracle.rand_field(rng, 2))
    gz = scale(zeta, root_of_unity(log_n))
    batches = [(zeta, [(k, 0, widths[k]) for k in range(n_or)])]
    sub = []
    for k in range(n_or):
        if rng.integers(0, 2):
            lo = int(rng.integers(0, widths[k]))
            hi = int(rng.integers(lo + 1, widths[k] + 1))
            sub.append((k, lo, hi))
    if sub:
        batches.append((gz, sub))
    return oracles, batches


# ---- the proof-of-work search beyond its first launch --------------------------------------------------------------------------------
POW_SCAN_BITS = 11
POW_LAUNCH_BITS = 12          # sipp_k_pow_search grinds 2^max(12, pow_bits + 1) nonces per launch: 2^12 at 11 bits


def pow_case(rule, s, pow_bits=POW_SCAN_BITS):
    """random_instance(4242, 10, 1, 4, ncols=(3, 2), salted=(False, False)) of tests/test_oracle_fri_generic.py behind the transcript
    prefix [s, 1, 2]"""
    return Case("pow-scan-rule%d-s%d" % (rule, s), widths=(3, 2), seed=4242, fri=dict(pow_bits=pow_bits, pow_rule=rule, num_queries=9),
                prefix=(s, 1, 2))


def pow_scan(rule, seeds=range(120)):
    """per launch class (0: the first launch holds the smallest witness, 1: the second, 2: a later one) the first prefix seed s whose
    smallest witness, by the oracle, lies there: {class: (s, witness)}"""
    inst = build(pow_case(rule, 0))
    found = {}
    for s in seeds:
        ch = _oracle.challenger([s, 1, 2])
        w = int(_oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, ch)[inst.witness_index()])
        found.setdefault(min(w >> POW_LAUNCH_BITS, 2), (s, w))
        if len(found) == 3:
            break
    return found


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    # opening points with special components (log_n 10: omega_{2n} has z^n = -1, and is no member of the trace subgroup)
    pts = {"base7": (7, 0), "imag7": (0, 7), "minus_one_nth": (root_of_unity(11), 0), "pm1_pm1": (P - 1, P - 1), "one_one": (1, 1)}
    for name, pt in pts.items():
        out.append(Case("points-" + name, widths=(2, 5), salted=(True, False), seed=101, point=pt))
    # the point zero: in the first batch alone, and in both
    all14, sub14 = all_columns((1, 4)), sub_columns((1, 4))
    out.append(Case("zero_point-first", widths=(1, 4), salted=(False, True), seed=102,
                    batches=lambda z, g: [((0, 0), all14), (scale(z, g), sub14)]))
    out.append(Case("zero_point-both", widths=(1, 4), salted=(False, True), seed=102, point=(0, 0)))
    # structured columns; an oracle that is zero altogether (its final polynomial and every FRI layer are zero)
    out.append(Case("structured", rate_bits=2, cap_height=3, widths=(10, 5), salted=(False, True), columns="structured", seed=103,
                    fri=dict(arity_bits=3, final_poly_bits=4)))
    out.append(Case("structured-all_zero", rate_bits=2, cap_height=3, widths=(3,), columns="zero", seed=104,
                    fri=dict(arity_bits=3, final_poly_bits=4)))
    # shape edges of the core
    out.append(Case("no_rounds", seed=105, fri=dict(arities=[])))
    out.append(Case("cap0", rate_bits=3, cap_height=0, seed=106))
    out.append(Case("cap8_last_layer-10", cap_height=8, seed=107, fri=dict(arities=[3])))           # 2^11 values / 8 = 2^8 leaves = the cap
    out.append(Case("cap8_last_layer-11", log_n=11, cap_height=8, seed=108, fri=dict(arities=[1, 3])))
    out.append(Case("queries-1", widths=(3,), seed=109, fri=dict(num_queries=1)))
    out.append(Case("queries-1024", widths=(3,), seed=109, fri=dict(num_queries=1024)))
    # eight oracles, leaves of 1 .. 4 words with and without salt (hash_or_noop's boundary from both sides), empty and repeated ranges
    w8 = (1, 2, 3, 4, 5, 8, 9, 17)

    def narrow_batches(z, g):
        return [(z, all_columns(w8)), (scale(z, g), [(7, 3, 3), (7, 16, 17), (2, 1, 2)]), (scale(z, g * g % P), [(0, 0, 1)]),
                (scale(z, pow(g, 3, P)), [(5, 0, 8), (5, 0, 8)])]
    for name, odd in (("odd_salted", 1), ("even_salted", 0)):
        out.append(Case("narrow-" + name, rate_bits=2, cap_height=3, widths=w8, salted=[k % 2 == odd for k in range(8)],
                        from_values=[k % 2 == 0 for k in range(8)], seed=110, batches=narrow_batches))
    # batches without a polynomial: one whose only range is empty, one with no range at all; and the first batch over again
    a32 = all_columns((3, 2))
    out.append(Case("empty_batch", widths=(3, 2), salted=(False, True), seed=111,
                    batches=lambda z, g: [(z, a32), (scale(z, g), [(0, 1, 1)]), (z, a32), (scale(z, g * g % P), [])]))
    # a challenger handed over with pending input (9 observations leave one), and with unread output on top
    out.append(Case("pending_challenger-in", seed=112, prefix=range(1, 10)))
    out.append(Case("pending_challenger-out", seed=112, prefix=range(1, 10), gets=1))
    for bits in (0, 11, 16):
        for rule in (0, 1):
            out.append(Case("pow-%d-rule%d" % (bits, rule), widths=(3, 2), seed=4242, fri=dict(pow_bits=bits, pow_rule=rule)))
    # sipp_k_openings in segments that do not divide n (59 segments of 1111 rows; 26 of 1261), idle lanes in the last trip
    out.append(Case("wide_ragged-35x16", log_n=16, widths=(35,), from_values=(False,), seed=113, fri=dict(num_queries=3),
                    batches=lambda z, g: [(z, [(0, 0, 35)]), (scale(z, g), [(0, 1, 34)])]))
    out.append(Case("wide_ragged-80x15", log_n=15, widths=(80,), from_values=(False,), seed=114, fri=dict(num_queries=3)))
    # 512 tiles in the division: two chunks of fri_divide_carry
    out.append(Case("long", log_n=19, widths=(2,), from_values=(False,), seed=115, fri=dict(num_queries=3)))
    for s in STRESS_SEEDS:
        out.append(Case("stress-%d" % s, stress_seed=s))
    return out


# eight configurations of the stress generator that the oracle proves and the GPU layer's documented range contains
# (mixed arities: 702, 711, 725, 743; cap_height 0: 702, 715; a salted oracle of at most 4 columns: 701, 702, 711, 712, 715;
#  ten rounds of arity 2 at blowup 8: 701; a final polynomial of one coefficient: 725; no proof of work: 705, 712)
STRESS_SEEDS = (701, 702, 705, 711, 712, 715, 725, 743)
CASES = _cases()
BY_ID = {c.id: c for c in CASES}
