#!/usr/bin/env python3
"""SIPP's transcript through the outer prover (sipp_amd/transcript.py SippTranscriptProver) over the fixture of n pairs
(tests/golden/sipp_n<n>_ios.npz; n = 4, 8, 128, ...):

    python scripts/perf_transcript_circuit.py [n]       # default 128

Prints one JSON line: the circuit's rows and levels, witness generation alone (sipp_plonk_generate_witness_levels on the circuit's
schedule, graph route), prove through the input cells and through the word map (witness + proof), verify; best of `reps`.  Needs the
oracle's hash for the public-inputs hash of the witness-only run (tests/_oracle.py, built by build())."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import sipp_amd
    from sipp_amd import transcript as tr
    from sipp_amd._lib import to_device
    from sipp_amd.circuit import fri_params
    from tests import _oracle
    from tests import _transcript_cases as tc
    st, rw, ex, d = tc.fixture(a.n)
    c = tr.SippTranscriptCircuit(a.n)
    gp, fp = sipp_amd.PlonkParams(80, 8, 2), fri_params(c.log_n)
    gc = sipp_amd.PlonkCircuit.from_dict(c.circuit())
    ctx = sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(c.log_n, C.byref(gp), C.byref(fp), C.byref(gc)))
    pr = tr.SippTranscriptProver(ctx, a.n, fri=fp, params=gp)
    ch = pr.challenges_of(d["fq12"])
    pis = c.public_inputs(st, rw, ch)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    cs = c.constants_sigmas()
    d_w, d_k = to_device(c.partial_witness(st, rw, ch)), to_device(cs[:c.num_constants])
    sched, gens = sipp_amd.PlonkSchedule.from_dict(c.schedule()), c.generators()
    wit, prove, words, verify = [], [], [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        ctx.plonk_generate_witness_levels(d_w, d_k, c.log_n, gens, pih, sched)
        wit.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pf = pr.prove(st, rw, ch)
        prove.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pw = pr.prove_words(st, rw, ch)
        words.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = pr.verify(pf)
        verify.append(time.perf_counter() - t0)
        assert ok == (0, 0) and (pw == pf).all(), ok
    assert pr.check_obligations(pis, d["g1"], d["g2"], d["fq12"])
    ms = lambda v: round(1e3 * min(v[1:]), 3)
    print(json.dumps({"n": a.n, "log_n": c.log_n, "rows_used": c.rows_used, "levels": c.n_levels, "transcript_rows": len(c.transcript_rows),
                      "public_inputs": c.n_pi, "witness_inputs": len(c.in_cycle), "witness_ms": ms(wit), "prove_ms": ms(prove),
                      "prove_words_ms": ms(words), "verify_ms": ms(verify), "proof_words": int(len(pf))}))
    pr.close()
    ctx.close()


if __name__ == "__main__":
    main()
