#!/usr/bin/env python3
"""Whole FRI query rounds through the outer prover at a recursion-shaped size (sipp_amd/fri_verifier.py FriVerifierProver): an opening
proof made by the device over an LDE of 2^log_m points (blowup 8, cap height 4, arity 16, the rounds ConstantArityBits(4, 5) gives) of
four oracles with the widths of a standard_ecc_config proof (constants and sigmas 84, wires 136, Z and partial products 20, quotient
chunks 16; everything opened at zeta, the third oracle at g zeta too), its `queries` query rounds proved and verified through one
CircuitData.  Run by hand.  Every GPU step is a child process under its own `timeout`:

    opening   the device's opening proof, read by tests/_fri_round_reading.py into the circuit's arguments (kept in a work file)
    witness   witness generation alone (sipp_plonk_generate_witness_levels on the circuit's schedule) per route, interleaved
    prove     prove through the dense call (sipp_circuit_prove) and through the input cells (sipp_circuit_prove_inputs), interleaved
              in one run, then verify

Prints one JSON line per step: the shape (rows used, N, public inputs, levels and how many of them the public-input chain sets), then
best, median and spread (max - min) of `reps`.  Needs the oracle for the transcript's start and the reading of the proof
(tests/_oracle.py; built by build())."""
import argparse
import ctypes as C
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = (84, 136, 20, 16)
RATE_BITS, CAP_HEIGHT = 3, 4
LIMITS = {"opening": 600, "witness": 300, "prove": 600}            # seconds, per step


def stats(v):
    v = v[1:]                                                       # the first repeat warms up
    return {"best_ms": round(1e3 * min(v), 3), "median_ms": round(1e3 * float(np.median(v)), 3), "spread_ms": round(1e3 * (max(v) - min(v)), 3)}


def opening(a):
    import sipp_amd
    from sipp_amd._lib import to_device
    from tests import _fri_cases as fc
    from tests import _fri_round_reading as rr
    from tests import _oracle
    from tests.test_gpu_fri_generic import gpu_challenger, to_params
    log_n = a.log_m - RATE_BITS
    case = fc.Case("perf", log_n=log_n, rate_bits=RATE_BITS, cap_height=CAP_HEIGHT, widths=WIDTHS,
                   fri=dict(arity_bits=4, final_poly_bits=5, num_queries=a.queries, pow_bits=16))
    ofp = fc.fri_params(case)
    rng = np.random.default_rng(13)
    zeta = tuple(int(x) for x in _oracle.rand_field(rng, 2))
    batches = [(zeta, fc.all_columns(WIDTHS)), (fc.scale(zeta, fc.root_of_unity(log_n)), [(2, 0, WIDTHS[2])])]
    ctx = sipp_amd.Ctx(workspace_bytes=8 << 30)
    ods, caps, keep = [], [], []
    for w in WIDTHS:
        od, cap, bufs = ctx.commit_ex(to_device(_oracle.rand_field(rng, (w, 1 << log_n))), log_n, RATE_BITS, CAP_HEIGHT)
        ods.append(od); caps.append(cap); keep.append(bufs)
    gch, _ = gpu_challenger(list(case.prefix))
    t0 = time.perf_counter()
    proof = ctx.fri_prove_openings(ods, batches, log_n, to_params(ofp), gch)
    t_open = time.perf_counter() - t0
    del ods, keep
    ctx.close()
    inst = types.SimpleNamespace(case=case, fp=ofp, log_n=log_n, batches=batches, n_salt=[0] * len(WIDTHS),
                                 oracles=[types.SimpleNamespace(ncols=w, n_salt=0, cap=cap) for w, cap in zip(WIDTHS, caps)])
    t0 = time.perf_counter()
    args, shape, _ = rr.round_data(inst, proof)                     # every Merkle path and every query checked in Python integers
    pickle.dump((args, shape), open(a.work, "wb"))
    print(json.dumps({"step": "opening", "opening_proof_words": int(len(proof)), "opening_prove_ms": round(1e3 * t_open, 3),
                      "reading_s": round(time.perf_counter() - t0, 2), "shape": [shape[0], shape[1], shape[2], [len(b) for b in shape[3]]] + list(shape[4:])}))


def circuit_of(a):
    from sipp_amd import fri_verifier as fv
    args, shape = pickle.load(open(a.work, "rb"))
    return fv, args, shape, fv.FriQueryRoundCircuit(*shape)


def describe(a):
    """the shape, on the host: how many levels only the public-input hash chain reaches tells what sets the schedule's depth"""
    _, args, _, circ = circuit_of(a)
    chain = set(circ.chain_row)
    others = 1 + max(int(circ.row_level[r]) for r in range(circ.rows_used) if r not in chain)
    cells, _ = circ.input_cells(*args)
    print(json.dumps({"step": "shape", "rows_used": circ.rows_used, "log_n": circ.log_n, "n": circ.n, "public_inputs": circ.n_pi,
                      "witness_inputs": len(circ.in_cycle), "input_cells": int(len(cells)), "table_cells": circ.num_wires * circ.n,
                      "levels": circ.n_levels, "levels_of_the_statement": others, "levels_only_the_public_input_chain_sets": circ.n_levels - others,
                      "k_base": circ.k_base, "k_ext": circ.k_ext}))


def witness(a):
    import sipp_amd
    from sipp_amd._lib import to_device
    from tests import _oracle
    _, args, _, circ = circuit_of(a)
    ctx = sipp_amd.Ctx(workspace_bytes=2 << 30)
    pis = circ.public_inputs(*args[:8])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    d_w, d_k = to_device(circ.partial_witness(*args)), to_device(circ.constants_sigmas()[:circ.num_constants])
    sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
    gens, L = circ.generators(), sipp_amd.lib()
    routes = {"graph": 0, "interp_one_lane": 16, "reduce_one_lane": 32, "no_graph": 4}          # SIPP_ROUTE_WITNESS_*
    wit = {name: [] for name in routes}
    for _ in range(a.reps + 1):
        for name, route in routes.items():                          # interleaved: every route sees the same clocks
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            ctx.plonk_generate_witness_levels(d_w, d_k, circ.log_n, gens, pih, sched)        # captures the route's graph
            t0 = time.perf_counter()
            ctx.plonk_generate_witness_levels(d_w, d_k, circ.log_n, gens, pih, sched)
            wit[name].append(time.perf_counter() - t0)
    assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
    print(json.dumps({"step": "witness", **{"witness_" + name: stats(v) for name, v in wit.items()}}))
    ctx.close()


def prove(a):
    import sipp_amd
    from sipp_amd import merkle as mk
    fv, args, shape, circ = circuit_of(a)
    gp, fp = sipp_amd.PlonkParams(80, 8, 2), mk.fri_params(circ.log_n)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    ctx = sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(fp), C.byref(gc)))
    pr = fv.FriVerifierProver(ctx, *shape, fri=fp, params=gp)
    pis = pr.circ.public_inputs(*args[:8])
    cells, values = pr.circ.input_cells(*args)
    dense_table = pr.circ.partial_witness(*args)
    dense, inputs, verify = [], [], []
    for _ in range(a.reps + 1):                                     # interleaved: both calls see the same clocks; host arrays made before
        t0 = time.perf_counter()
        pf_d = pr.data.prove(dense_table, pis)
        dense.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pf_i = pr.data.prove_inputs(cells, values, pis)
        inputs.append(time.perf_counter() - t0)
        assert len(pf_d) == len(pf_i) and (pf_d == pf_i).all()
        t0 = time.perf_counter()
        ok = pr.verify(pf_i)
        verify.append(time.perf_counter() - t0)
        assert ok == (0, 0), ok
    print(json.dumps({"step": "prove", "prove_dense": stats(dense), "prove_inputs": stats(inputs), "verify": stats(verify),
                      "dense_table_bytes": int(dense_table.nbytes), "input_pair_bytes": int(cells.nbytes + values.nbytes), "proof_words": int(len(pf_i))}))
    pr.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=28)
    ap.add_argument("--log-m", type=int, default=21)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step", choices=["opening", "witness", "prove"], help="run one step in this process (what the parent starts)")
    ap.add_argument("--work", help="the work file between the steps")
    a = ap.parse_args()
    if a.step:
        return {"opening": opening, "witness": witness, "prove": prove}[a.step](a)
    with tempfile.TemporaryDirectory() as tmp:
        a.work = os.path.join(tmp, "arguments.pickle")
        common = [sys.executable, os.path.abspath(__file__), "--queries", str(a.queries), "--log-m", str(a.log_m), "--reps", str(a.reps), "--work", a.work]
        for step in ("opening", "witness", "prove"):
            # a step that faults, aborts or runs out of time ends the run: nothing more is started on the card
            subprocess.check_call(["timeout", "-k", "10", str(LIMITS[step])] + common + ["--step", step])
            if step == "opening":
                describe(a)


if __name__ == "__main__":
    main()
