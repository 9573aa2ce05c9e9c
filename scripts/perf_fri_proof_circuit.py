#!/usr/bin/env python3
"""The whole FRI verifier through the outer prover at a recursion-shaped size (sipp_amd/fri_proof.py FriProofProver) beside the
query-round circuit it grew from (sipp_amd/fri_verifier.py FriVerifierProver), on the opening proof of
scripts/perf_fri_verifier_circuit.py: an LDE of 2^log_m points (blowup 8, cap height 4, arity 16, the rounds ConstantArityBits(4, 5)
gives), four oracles of 84 / 136 / 20 / 16 columns, `queries` queries, 16 bits of proof of work.  Run by hand.  Every GPU step is a child
process under its own `timeout`, the steps are chained, and nothing starts after a failure:

    opening   the device's opening proof; kept in a work file with its caps, points and arriving transcript, and with the arguments
              tests/_fri_round_reading.py reads of it for the query-round circuit (that reading is timed)
    witness   witness generation alone (sipp_plonk_generate_witness_levels) of both circuits, interleaved
    prove     FriProofProver.prove_proof and FriVerifierProver.prove, interleaved in one run, each verified; and the host time from the
              flat proof to the (cell, value) pairs on both ways

Prints one JSON line per step: the shapes (rows, levels, how many levels the transcript sets), then best, median and spread (max - min)
of `reps`.  Needs the oracle for the readings (tests/_oracle.py; built by build())."""
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
RATE_BITS, CAP_HEIGHT, POW_BITS = 3, 4, 16
LIMITS = {"opening": 600, "witness": 300, "prove": 600}            # seconds, per step


def stats(v):
    v = v[1:]                                                       # the first repeat warms up
    return {"best_ms": round(1e3 * min(v), 3), "median_ms": round(1e3 * float(np.median(v)), 3), "spread_ms": round(1e3 * (max(v) - min(v)), 3)}


def opening(a):
    import sipp_amd
    from sipp_amd._lib import to_device
    from tests import _challenger_reading as cr
    from tests import _fri_cases as fc
    from tests import _fri_round_reading as rr
    from tests import _oracle
    from tests.test_gpu_fri_generic import gpu_challenger, to_params
    log_n = a.log_m - RATE_BITS
    case = fc.Case("perf", log_n=log_n, rate_bits=RATE_BITS, cap_height=CAP_HEIGHT, widths=WIDTHS,
                   fri=dict(arity_bits=4, final_poly_bits=5, num_queries=a.queries, pow_bits=POW_BITS))
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
    args, shape, data = rr.round_data(inst, proof)                  # every Merkle path and every query checked in Python integers
    t_read = time.perf_counter() - t0
    pickle.dump({"proof": np.asarray(proof, dtype=np.uint64), "caps": data["caps"], "points": data["points"],
                 "transcript": cr.arriving(case)[0], "round_args": args, "shape": shape}, open(a.work, "wb"))
    print(json.dumps({"step": "opening", "opening_proof_words": int(len(proof)), "opening_prove_ms": round(1e3 * t_open, 3),
                      "reading_s": round(t_read, 2), "shape": [shape[0], shape[1], shape[2], [len(b) for b in shape[3]]] + list(shape[4:])}))


def circuits_of(a):
    from sipp_amd import fri_proof as fp
    from sipp_amd import fri_verifier as fv
    o = pickle.load(open(a.work, "rb"))
    kw = dict(pow_bits=POW_BITS, pow_rule=0, n_in=len(o["transcript"][1]))
    return o, kw, fp.FriProofCircuit(*o["shape"], **kw), fv.FriQueryRoundCircuit(*o["shape"])


def describe(a):
    """the shapes, on the host: what the transcript in circuit costs in rows and levels"""
    o, _, whole, rounds = circuits_of(a)
    cells, _ = whole.input_map()
    line = {"step": "shape"}
    for name, c in (("fri_proof", whole), ("fri_verifier", rounds)):
        chain = set(c.chain_row)
        others = 1 + max(int(c.row_level[r]) for r in range(c.rows_used) if r not in chain)
        line[name] = {"rows_used": c.rows_used, "log_n": c.log_n, "public_inputs": c.n_pi, "witness_inputs": len(c.in_cycle),
                      "levels": c.n_levels, "levels_of_the_statement": others}
    line["fri_proof"].update({"levels_the_transcript_sets": whole.transcript_levels, "transcript_rows": len(whole.transcript_row),
                              "input_cells_from_proof_words": int(len(cells)), "generators": len(whole.generators())})
    print(json.dumps(line))


def witness(a):
    import sipp_amd
    from sipp_amd._lib import to_device
    from sipp_amd import fri_proof as fp
    from tests import _oracle
    o, _, whole, rounds = circuits_of(a)
    ctx = sipp_amd.Ctx(workspace_bytes=2 << 30)
    runs = {}
    for name, c, args, n_pub in (("fri_proof", whole, fp.flat_proof_arguments(whole, o["proof"], o["caps"], o["points"], o["transcript"]), 6),
                                 ("fri_verifier", rounds, o["round_args"], 8)):
        pih = _oracle.hash_no_pad(np.array(c.public_inputs(*args[:n_pub]), dtype=np.uint64))
        runs[name] = (c, to_device(c.partial_witness(*args)), to_device(c.constants_sigmas()[:c.num_constants]),
                      sipp_amd.PlonkSchedule.from_dict(c.schedule()), pih)
    wit = {name: [] for name in runs}
    for _ in range(a.reps + 1):
        for name, (c, d_w, d_k, sched, pih) in runs.items():       # interleaved: both circuits see the same clocks
            ctx.plonk_generate_witness_levels(d_w, d_k, c.log_n, c.generators(), pih, sched)       # captures this circuit's graph
            t0 = time.perf_counter()
            ctx.plonk_generate_witness_levels(d_w, d_k, c.log_n, c.generators(), pih, sched)
            wit[name].append(time.perf_counter() - t0)
    print(json.dumps({"step": "witness", **{"witness_" + name: stats(v) for name, v in wit.items()}}))
    ctx.close()


def prove(a):
    import sipp_amd
    from sipp_amd import fri_proof as fp
    from sipp_amd import fri_verifier as fv
    from sipp_amd import merkle as mk
    o, kw, whole, rounds = circuits_of(a)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    provers, ctxs = {}, []
    for name, c in (("fri_proof", whole), ("fri_verifier", rounds)):
        f = mk.fri_params(c.log_n)
        gc = sipp_amd.PlonkCircuit.from_dict(c.circuit())
        ctx = sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(c.log_n, C.byref(gp), C.byref(f), C.byref(gc)))
        ctxs.append(ctx)
        provers[name] = (fp.FriProofProver(ctx, *o["shape"], fri=f, params=gp, **kw) if name == "fri_proof" else
                         fv.FriVerifierProver(ctx, *o["shape"], fri=f, params=gp))
    new, old = provers["fri_proof"], provers["fri_verifier"]
    t = {k: [] for k in ("prove_proof", "verify_fri_proof", "prove_fri_verifier", "verify_fri_verifier", "host_proof_inputs", "host_input_cells")}
    for _ in range(a.reps + 1):                                     # interleaved: both provers see the same clocks
        t0 = time.perf_counter()
        pf_n = new.prove_proof(o["proof"], o["caps"], o["points"], o["transcript"])
        t["prove_proof"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = new.verify(pf_n)
        t["verify_fri_proof"].append(time.perf_counter() - t0)
        assert ok == (0, 0), ok
        t0 = time.perf_counter()
        pf_o = old.prove(*o["round_args"])
        t["prove_fri_verifier"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = old.verify(pf_o)
        t["verify_fri_verifier"].append(time.perf_counter() - t0)
        assert ok == (0, 0), ok
        # the host's part of either call: from the flat proof (here: from the arguments read of it, the opening step's reading_s
        # comes on top) to the (cell, value) pairs
        t0 = time.perf_counter()
        new.circ.proof_inputs(o["proof"], o["caps"], o["points"], o["transcript"])
        t["host_proof_inputs"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        old.circ.input_cells(*o["round_args"])
        t["host_input_cells"].append(time.perf_counter() - t0)
    print(json.dumps({"step": "prove", **{k: stats(v) for k, v in t.items()}, "proof_words": [int(len(pf_n)), int(len(pf_o))]}))
    for pr in provers.values():
        pr.close()
    for ctx in ctxs:
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
        a.work = os.path.join(tmp, "opening.pickle")
        common = [sys.executable, os.path.abspath(__file__), "--queries", str(a.queries), "--log-m", str(a.log_m), "--reps", str(a.reps), "--work", a.work]
        for step in ("opening", "witness", "prove"):
            # a step that faults, aborts or runs out of time ends the run: nothing more is started on the card
            subprocess.check_call(["timeout", "-k", "10", str(LIMITS[step])] + common + ["--step", step])
            if step == "opening":
                describe(a)


if __name__ == "__main__":
    main()
