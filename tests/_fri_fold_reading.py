"""A Python reading of the three generators of a FRI fold chain (SIPP_GEN_ARITHMETIC_EXT, SIPP_GEN_EXPONENTIATION,
SIPP_GEN_COSET_INTERPOLATION) in exact integers, row by row, and of the data a fold-checking circuit is fed: the checker of the device
witness of sipp_amd/fri_fold.py.  It shares nothing with that module or the kernels: the layouts are restated from include/sipp_hip.h, the
barycentric weights are computed from their product definition 1 / prod_(j != i) (x_i - x_j).  tests/_witness_reading.py runs the row
functions on the rows that hold their generators.

fold_data(inst, proof) walks a flat opening proof (sipp_fri_prove_openings / oracle/fri.c) the way
tests/test_oracle_fri_edges.py::python_reading_accepts does and returns what the circuit takes: betas, the final polynomial, per query
(x_index, the first `old`, the evals of every round)."""
from oracle.py import plonky2_generic as g2

P = 0xFFFFFFFF00000001
ROOT32 = 1753635133440165772


def inv(a):
    """a^(p - 2): inv(0) = 0, as the device's gl::inv"""
    return pow(a, P - 2, P)


def emul(x, y, W):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


_DOMAIN = {}


def domain(s):
    """(points x_i = g^i of the subgroup of order 2^s, weights 1 / prod_(j != i) (x_i - x_j))"""
    if s not in _DOMAIN:
        g = pow(ROOT32, 1 << (32 - s), P)
        xs = [pow(g, i, P) for i in range(1 << s)]
        ws = []
        for i, xi in enumerate(xs):
            den = 1
            for j, xj in enumerate(xs):
                if j != i:
                    den = den * (xi - xj) % P
            ws.append(inv(den))
        _DOMAIN[s] = (xs, ws)
    return _DOMAIN[s]


def arithmetic_ext_row(w, c0, c1, n_ops, W):
    """w: the row's wires as a list of ints, in place"""
    for k in range(n_ops):
        b = 8 * k
        m = emul((w[b], w[b + 1]), (w[b + 2], w[b + 3]), W)
        w[b + 6] = (c0 * m[0] + c1 * w[b + 4]) % P
        w[b + 7] = (c0 * m[1] + c1 * w[b + 5]) % P


def exponentiation_row(w, n_bits):
    base, prev = w[0], 1
    for i in range(n_bits):
        bit = w[n_bits - i]
        prev = prev * prev * (bit * base + 1 - bit) % P
        w[2 + n_bits + i] = prev
    w[1 + n_bits] = prev


def coset_interpolation_row(w, s, d, W):
    n = 1 << s
    ni = (n - 2) // (d - 1)
    start = 1 + 2 * n + 4
    xs, ws = domain(s)
    si = inv(w[0])
    sh = (w[1 + 2 * n] * si % P, w[2 + 2 * n] * si % P)
    w[start + 4 * ni], w[start + 4 * ni + 1] = sh
    e, q = (0, 0), (1, 0)
    chunk_end = [min(d, n)]
    while chunk_end[-1] < n:
        chunk_end.append(min(n, chunk_end[-1] + d - 1))
    assert len(chunk_end) == ni + 1
    for i in range(n):
        t = ((sh[0] - xs[i]) % P, sh[1])
        vw = (w[1 + 2 * i] * ws[i] % P, w[2 + 2 * i] * ws[i] % P)
        et, vq = emul(e, t, W), emul(vw, q, W)
        e, q = ((et[0] + vq[0]) % P, (et[1] + vq[1]) % P), emul(q, t, W)
        if i + 1 in chunk_end[:-1]:
            c = chunk_end.index(i + 1)
            w[start + 2 * c], w[start + 2 * c + 1] = e
            w[start + 2 * ni + 2 * c], w[start + 2 * ni + 2 * c + 1] = q
    w[3 + 2 * n], w[4 + 2 * n] = e


def fold_data(inst, proof):
    """(betas, final_poly, queries) of a flat opening proof of the tests/_fri_cases instance: queries = [(x_index, old, evals per round)],
    ext values as (c0, c1); the first `old` by the arithmetic of fri_verify_query (fri_combine_initial, times x); every query is accepted
    by fri_verify_query"""
    case, fp, log_n = inst.case, inst.fp, inst.log_n
    pf = [int(x) for x in proof]
    arities = [fp.arity_bits[i] for i in range(fp.n_rounds)]
    log_m = log_n + fp.rate_bits
    pos = [8]

    def take(k):
        v = pf[pos[0]:pos[0] + k]
        assert len(v) == k
        pos[0] += k
        return v
    ch = g2.Challenger()
    ch.observe_many([case.stress_seed, 1, 2] if case.stress_seed is not None else list(case.prefix))
    for _ in range(case.gets):
        ch.get()
    opened = []
    for pt, ranges in inst.batches:
        vals = [g2.Ext(*take(2)) for _ in range(sum(e - b for _, b, e in ranges))]
        for v in vals:
            ch.observe_ext(v)
        opened.append(vals)
    alpha = ch.get_ext()
    caps, betas = [], []
    for _ in arities:
        caps.append([take(4) for _ in range(1 << fp.cap_height)])
        ch.observe_cap(caps[-1])
        betas.append(ch.get_ext())
    final_poly = [g2.Ext(*take(2)) for _ in range((1 << log_n) >> sum(arities))]
    for c in final_poly:
        ch.observe_ext(c)
    take(1)                                                          # the proof-of-work witness: not this circuit's
    g2.pow_response(ch, fp.pow_rule, pf[pos[0] - 1])
    queries = []
    for _ in range(fp.num_queries):
        x = ch.get() % (1 << log_m)
        rows = []
        for o in inst.oracles:
            row = take(o.ncols + o.n_salt)
            take(4 * (log_m - fp.cap_height))
            rows.append(row)
        steps = []
        for r, ab in enumerate(arities):
            ev = take(2 << ab)
            take(4 * max(0, log_m - sum(arities[:r + 1]) - fp.cap_height))
            steps.append([g2.Ext(ev[2 * k], ev[2 * k + 1]) for k in range(1 << ab)])
        fb = []
        for (pt, ranges), vals in zip(inst.batches, opened):
            at_x = [rows[o][c] for o, b, e in ranges for c in range(b, e)]
            fb.append((g2.Ext(*pt), at_x, vals))
        assert g2.fri_verify_query(x, log_n, fp.rate_bits, arities, alpha, fb, rows, steps, betas, final_poly) is None
        # the first old: fri_combine_initial, times x
        sx = g2.GEN * pow(g2.primitive_root_of_unity(log_m), g2.reverse_bits(x, log_m), P) % P
        total = g2.Ext(0)
        for point, at_x, vals in fb:
            acc_x, acc_o = g2.Ext(0), g2.Ext(0)
            for v, o in zip(reversed(at_x), reversed(vals)):
                acc_x = acc_x * alpha + v
                acc_o = acc_o * alpha + o
            total = total * (alpha ** len(at_x)) + (acc_x - acc_o) * (g2.Ext(sx) - point).inverse()
        old = total * sx
        assert old == steps[0][x & ((1 << arities[0]) - 1)]
        queries.append((x, (int(old[0]), int(old[1])), [[(int(v[0]), int(v[1])) for v in st] for st in steps]))
    assert pos[0] == len(pf)
    return [(int(b[0]), int(b[1])) for b in betas], [(int(c[0]), int(c[1])) for c in final_poly], queries
