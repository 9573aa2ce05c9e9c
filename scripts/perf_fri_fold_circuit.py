#!/usr/bin/env python3
"""FRI fold chains through the outer prover at a recursion-shaped size (sipp_amd/fri_fold.py FriFoldProver): an opening proof made by the
device over an LDE of 2^log_m points (blowup 8, arity 16, the rounds ConstantArityBits(4, 5) gives), its `queries` fold chains proved and
verified through one CircuitData.  Prints one JSON line: witness generation alone (sipp_plonk_generate_witness_levels on the circuit's
schedule, graph route) with the sixteen-lane interpolation and with SIPP_ROUTE_WITNESS_INTERP_ONE_LANE -- interleaved in the same run, best
of `reps` -- then prove (host to host) and verify.  Needs the oracle for the transcript's start and the reading of the proof
(tests/_oracle.py, tests/_fri_fold_reading.py; built by build())."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=28)
    ap.add_argument("--log-m", type=int, default=21)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import sipp_amd
    from sipp_amd import fri_fold as ff
    from sipp_amd import merkle as mk
    from sipp_amd._lib import to_device
    from tests import _fri_cases as fc
    from tests import _fri_fold_reading as fr
    from tests import _oracle
    from tests.test_gpu_fri_generic import gpu_challenger, to_params
    rate_bits, cap_h, widths = 3, 4, (4,)
    log_n = a.log_m - rate_bits
    case = fc.Case("perf", log_n=log_n, rate_bits=rate_bits, cap_height=cap_h, widths=widths,
                   fri=dict(arity_bits=4, final_poly_bits=5, num_queries=a.queries, pow_bits=16))
    ofp = fc.fri_params(case)
    rng = np.random.default_rng(9)
    zeta = tuple(int(x) for x in _oracle.rand_field(rng, 2))
    batches = [(zeta, fc.all_columns(widths))]
    # the opening proof, made by the device
    ctx0 = sipp_amd.Ctx(workspace_bytes=4 << 30)
    od, _cap, _keep = ctx0.commit_ex(to_device(_oracle.rand_field(rng, (widths[0], 1 << log_n))), log_n, rate_bits, cap_h)
    gch, _ = gpu_challenger(list(case.prefix))
    opening = ctx0.fri_prove_openings([od], batches, log_n, to_params(ofp), gch)
    inst = types.SimpleNamespace(case=case, fp=ofp, log_n=log_n, batches=batches, oracles=[types.SimpleNamespace(ncols=widths[0], n_salt=0)])
    betas, final_poly, queries = fr.fold_data(inst, opening)
    del od, _keep
    ctx0.close()
    shape = (a.log_m, 4, ofp.n_rounds, len(final_poly), a.queries)
    fcirc = ff.FriFoldCircuit(*shape)
    gp, fp = sipp_amd.PlonkParams(80, 8, 2), mk.fri_params(fcirc.log_n)
    gc = sipp_amd.PlonkCircuit.from_dict(fcirc.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(fcirc.log_n, C.byref(gp), C.byref(fp), C.byref(gc))
    ctx = sipp_amd.Ctx(workspace_bytes=ws)
    pr = ff.FriFoldProver(ctx, *shape, fri=fp, params=gp)
    pis = fcirc.public_inputs(betas, final_poly, queries)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    cs = fcirc.constants_sigmas()
    d_w, d_k = to_device(fcirc.partial_witness(betas, final_poly, queries)), to_device(cs[:6])
    sched = sipp_amd.PlonkSchedule.from_dict(fcirc.schedule())
    gens = fcirc.generators()
    L = sipp_amd.lib()
    ONE_LANE = 16                                  # SIPP_ROUTE_WITNESS_INTERP_ONE_LANE
    wit = {0: [], ONE_LANE: []}
    for _ in range(a.reps + 1):
        for route in (0, ONE_LANE):                       # interleaved: both forms see the same clocks
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            ctx.plonk_generate_witness_levels(d_w, d_k, fcirc.log_n, gens, pih, sched)      # captures the route's graph
            t0 = time.perf_counter()
            ctx.plonk_generate_witness_levels(d_w, d_k, fcirc.log_n, gens, pih, sched)
            wit[route].append(time.perf_counter() - t0)
    assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
    prove, verify = [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        pf = pr.prove(betas, final_poly, queries)
        prove.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = pr.verify(pf)
        verify.append(time.perf_counter() - t0)
        assert ok == (0, 0), ok
    ms = lambda v: round(1e3 * min(v[1:]), 3)
    med = lambda v: round(1e3 * float(np.median(v[1:])), 3)
    print(json.dumps({"queries": a.queries, "log_m": a.log_m, "arity_bits": 4, "rounds": int(ofp.n_rounds), "final_len": len(final_poly),
                      "log_n": fcirc.log_n, "rows_used": fcirc.rows_used, "levels": fcirc.n_levels, "public_inputs": fcirc.n_pi,
                      "witness_sixteen_lane_ms": ms(wit[0]), "witness_one_lane_ms": ms(wit[ONE_LANE]),
                      "witness_sixteen_lane_median_ms": med(wit[0]), "witness_one_lane_median_ms": med(wit[ONE_LANE]),
                      "prove_ms": ms(prove), "verify_ms": ms(verify), "prove_plus_verify_ms": round(ms(prove) + ms(verify), 3),
                      "proof_words": int(len(pf))}))
    pr.close()
    ctx.close()


if __name__ == "__main__":
    main()
