"""A Python reading of the generators of FRI's initial combination (SIPP_GEN_REDUCING, SIPP_GEN_REDUCING_EXT, SIPP_GEN_QUOTIENT_EXT) in
exact integers, row by row, and of the data a circuit that checks fri_combine_initial is fed: the checker of the device witness of
sipp_amd/fri_initial.py.  It shares nothing with that module or the kernels: the layouts are restated from include/sipp_hip.h.
tests/_witness_reading.py runs the row functions on the rows that hold their generators.

initial_data(inst, proof) walks a flat opening proof (sipp_fri_prove_openings / oracle/fri.c) the way tests/_fri_fold_reading.fold_data
does and returns what the circuit takes: alpha, per batch the point and the opened values, per query (x_index, the unsalted leaf values
of every oracle in a row, the `old` that enters the first fold), and the column lists of the batches."""
import numpy as np

from oracle.py import plonky2_generic as g2
from tests import _fri_fold_reading as fr

P = 0xFFFFFFFF00000001


def ext_inv(x, W):
    """(x0 - x1 X) / (x0^2 - W x1^2), with inv(0) = 0"""
    ni = fr.inv((x[0] * x[0] - W * x[1] * x[1]) % P)
    return (x[0] * ni % P, (P - x[1]) % P * ni % P)


def reducing_row(w, K, W):
    """alpha 0, old acc 2, K base coefficients from 4, K accumulators (2 each) from 4 + K"""
    alpha, acc = (w[0], w[1]), (w[2], w[3])
    for i in range(K):
        m = fr.emul(acc, alpha, W)
        acc = ((m[0] + w[4 + i]) % P, m[1])
        w[4 + K + 2 * i], w[5 + K + 2 * i] = acc


def reducing_ext_row(w, K, W):
    """alpha 0, old acc 2, K extension coefficients (2 each) from 4, K accumulators (2 each) from 4 + 2K"""
    alpha, acc = (w[0], w[1]), (w[2], w[3])
    for i in range(K):
        m = fr.emul(acc, alpha, W)
        acc = ((m[0] + w[4 + 2 * i]) % P, (m[1] + w[5 + 2 * i]) % P)
        w[4 + 2 * K + 2 * i], w[5 + 2 * K + 2 * i] = acc


def quotient_ext_row(w, c0, c1, n_ops, W):
    """per op at b = 8k: the multiplicand (b+2, b+3) = (out - c1 c) inv(c0 a), read from a (b), c (b+4), out (b+6)"""
    for k in range(n_ops):
        b = 8 * k
        num = ((w[b + 6] - c1 * w[b + 4]) % P, (w[b + 7] - c1 * w[b + 5]) % P)
        den = (c0 * w[b] % P, c0 * w[b + 1] % P)
        w[b + 2], w[b + 3] = fr.emul(num, ext_inv(den, W), W)


def initial_data(inst, proof):
    """(alpha, points, opened, queries, batches, n_columns) of a flat opening proof of the tests/_fri_cases instance: queries =
    [(x_index, leaf values, old)], batches = per batch the column indices into a query's leaf values, ext values as (c0, c1); `old` by
    plonky2_generic's arithmetic (fri_combine_initial, times x); every query is accepted by fri_verify_query"""
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
    betas = []
    for _ in arities:
        ch.observe_cap([take(4) for _ in range(1 << fp.cap_height)])
        betas.append(ch.get_ext())
    final_poly = [g2.Ext(*take(2)) for _ in range((1 << log_n) >> sum(arities))]
    for c in final_poly:
        ch.observe_ext(c)
    take(1)                                                          # the proof-of-work witness: not this circuit's
    g2.pow_response(ch, fp.pow_rule, pf[pos[0] - 1])
    first = np.cumsum([0] + [o.ncols for o in inst.oracles])         # an oracle's first column in the row of unsalted leaf values
    batches = [[int(first[o]) + c for o, b, e in ranges for c in range(b, e)] for _, ranges in inst.batches]
    queries = []
    for _ in range(fp.num_queries):
        x = ch.get() % (1 << log_m)
        rows = []
        for o in inst.oracles:
            rows.append(take(o.ncols + o.n_salt))
            take(4 * (log_m - fp.cap_height))
        steps = []
        for r, ab in enumerate(arities):
            ev = take(2 << ab)
            take(4 * max(0, log_m - sum(arities[:r + 1]) - fp.cap_height))
            steps.append([g2.Ext(ev[2 * k], ev[2 * k + 1]) for k in range(1 << ab)])
        leaves = [v for o, row in zip(inst.oracles, rows) for v in row[:o.ncols]]
        fb = []
        for (pt, ranges), vals, cols in zip(inst.batches, opened, batches):
            at_x = [rows[o][c] for o, b, e in ranges for c in range(b, e)]
            assert at_x == [leaves[c] for c in cols]
            fb.append((g2.Ext(*pt), at_x, vals))
        assert g2.fri_verify_query(x, log_n, fp.rate_bits, arities, alpha, fb, rows, steps, betas, final_poly) is None
        sx = g2.GEN * pow(g2.primitive_root_of_unity(log_m), g2.reverse_bits(x, log_m), P) % P
        total = g2.Ext(0)
        for point, at_x, vals in fb:
            acc_x, acc_o = g2.Ext(0), g2.Ext(0)
            for v, o in zip(reversed(at_x), reversed(vals)):
                acc_x = acc_x * alpha + v
                acc_o = acc_o * alpha + o
            total = total * (alpha ** len(at_x)) + (acc_x - acc_o) * (g2.Ext(sx) - point).inverse()
        old = total * sx
        queries.append((x, leaves, (int(old[0]), int(old[1]))))
    assert pos[0] == len(pf)
    pair = lambda v: (int(v[0]), int(v[1]))
    return (pair(alpha), [pair(g2.Ext(*pt)) for pt, _ in inst.batches], [[pair(v) for v in vals] for vals in opened], queries, batches,
            int(first[-1]))
