#!/usr/bin/env python3
"""FRI's initial combination through the outer prover at a recursion-shaped size (sipp_amd/fri_initial.py FriInitialProver): `queries`
queries over an LDE of 2^log_m points, a zeta batch of `columns` leaf values and a g zeta batch of 2.  The circuit checks the combination
alone (no Merkle path, no fold), so the inputs are random field values and the `old` of every query is computed here in Python integers.
Prints one JSON line: witness generation alone (sipp_plonk_generate_witness_levels on the circuit's schedule, graph route) with the
sixteen-lane reduction and with SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE -- interleaved in the same run; best, median and spread (max - min) of
`reps` -- then prove (host to host) and verify.  Needs the oracle for the public-inputs hash (tests/_oracle.py; built by build())."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 0xFFFFFFFF00000001
W = 7


def emul(x, y):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def einv(x):
    ni = pow((x[0] * x[0] - W * x[1] * x[1]) % P, P - 2, P)
    return (x[0] * ni % P, (P - x[1]) * ni % P)


def combine(log_m, alpha, points, opened, batches, x_index, leaves):
    """fri_combine_initial, times x"""
    rev = int(format(x_index, "0%db" % log_m)[::-1], 2)
    x = 7 * pow(pow(1753635133440165772, 1 << (32 - log_m), P), rev, P) % P
    total = (0, 0)
    for pt, vals, cols in zip(points, opened, batches):
        acc_x, acc_o, al = (0, 0), (0, 0), (1, 0)
        for c, o in zip(reversed(cols), reversed(vals)):
            m = emul(acc_x, alpha)
            acc_x = ((m[0] + leaves[c]) % P, m[1])
            m = emul(acc_o, alpha)
            acc_o = ((m[0] + o[0]) % P, (m[1] + o[1]) % P)
            al = emul(al, alpha)
        num = ((acc_x[0] - acc_o[0]) % P, (acc_x[1] - acc_o[1]) % P)
        quot = emul(num, einv(((x - pt[0]) % P, (P - pt[1]) % P)))
        m = emul(total, al)
        total = ((m[0] + quot[0]) % P, (m[1] + quot[1]) % P)
    return emul(total, (x, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=28)
    ap.add_argument("--log-m", type=int, default=21)
    ap.add_argument("--columns", type=int, default=257)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import sipp_amd
    from sipp_amd import fri_initial as fi
    from sipp_amd import merkle as mk
    from sipp_amd._lib import to_device
    from tests import _oracle
    rng = np.random.default_rng(11)
    ext = lambda: tuple(int(v) for v in _oracle.rand_field(rng, 2))
    batches = [list(range(a.columns)), [0, 1]]
    alpha, points = ext(), [ext(), ext()]
    opened = [[ext() for _ in b] for b in batches]
    queries = []
    for _ in range(a.queries):
        x_index = int(rng.integers(0, 1 << a.log_m))
        leaves = [int(v) for v in _oracle.rand_field(rng, a.columns)]
        queries.append((x_index, leaves, combine(a.log_m, alpha, points, opened, batches, x_index, leaves)))
    shape = (a.log_m, a.columns, batches, a.queries)
    circ = fi.FriInitialCircuit(*shape)
    gp, fp = sipp_amd.PlonkParams(80, 8, 2), mk.fri_params(circ.log_n)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(fp), C.byref(gc))
    ctx = sipp_amd.Ctx(workspace_bytes=ws)
    pr = fi.FriInitialProver(ctx, *shape, fri=fp, params=gp)
    args = (alpha, points, opened, queries)
    pis = circ.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    cs = circ.constants_sigmas()
    d_w, d_k = to_device(circ.partial_witness(*args)), to_device(cs[:5])
    sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
    gens = circ.generators()
    L = sipp_amd.lib()
    ONE_LANE = 32                                  # SIPP_ROUTE_WITNESS_REDUCE_ONE_LANE
    wit = {0: [], ONE_LANE: []}
    for _ in range(a.reps + 1):
        for route in (0, ONE_LANE):                       # interleaved: both forms see the same clocks
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            ctx.plonk_generate_witness_levels(d_w, d_k, circ.log_n, gens, pih, sched)       # captures the route's graph
            t0 = time.perf_counter()
            ctx.plonk_generate_witness_levels(d_w, d_k, circ.log_n, gens, pih, sched)
            wit[route].append(time.perf_counter() - t0)
    assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
    prove, verify = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        pf = pr.prove(*args)
        prove.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = pr.verify(pf)
        verify.append(time.perf_counter() - t0)
        assert ok == (0, 0), ok
    ms = lambda v: round(1e3 * min(v[1:]), 3)
    med = lambda v: round(1e3 * float(np.median(v[1:])), 3)
    spread = lambda v: round(1e3 * (max(v[1:]) - min(v[1:])), 3)
    print(json.dumps({"queries": a.queries, "log_m": a.log_m, "batches": [len(b) for b in batches], "k_base": circ.k_base, "k_ext": circ.k_ext,
                      "log_n": circ.log_n, "rows_used": circ.rows_used, "levels": circ.n_levels, "public_inputs": circ.n_pi,
                      "witness_sixteen_lane_ms": ms(wit[0]), "witness_one_lane_ms": ms(wit[ONE_LANE]),
                      "witness_sixteen_lane_median_ms": med(wit[0]), "witness_one_lane_median_ms": med(wit[ONE_LANE]),
                      "witness_sixteen_lane_spread_ms": spread(wit[0]), "witness_one_lane_spread_ms": spread(wit[ONE_LANE]),
                      "prove_ms": ms(prove), "verify_ms": ms(verify), "prove_plus_verify_ms": round(ms(prove) + ms(verify), 3),
                      "proof_words": int(len(pf))}))
    pr.close()
    ctx.close()


if __name__ == "__main__":
    main()
