#!/usr/bin/env python3
"""Merkle openings through the outer prover at a recursion-shaped size (sipp_amd/merkle.py MerkleOpeningProver): a device commitment of
2^(log_leaves) leaves (cap height 4), `paths` openings of height log_leaves - 4 proved and verified through one CircuitData.  Prints one JSON
line: witness generation alone (sipp_plonk_generate_witness_levels on the circuit's schedule, graph route), prove (witness + proof) and
verify, best of `reps`, with the circuit's rows and levels.  Needs the oracle's tree for the siblings (tests/_oracle.py, built by build())."""
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
    ap.add_argument("--paths", type=int, default=128)
    ap.add_argument("--log-leaves", type=int, default=20)
    ap.add_argument("--leaf-len", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import sipp_amd
    from sipp_amd import merkle as mk
    from sipp_amd._lib import to_device
    from tests import _merkle_reading as mr
    from tests import _oracle
    cap_h, log_n_tree = 4, a.log_leaves - 1
    height = a.log_leaves - cap_h
    rng = np.random.default_rng(7)
    cols = _oracle.rand_field(rng, (a.leaf_len, 1 << log_n_tree))
    b = _oracle.Batch(cols, log_n_tree, rate_bits=1, cap_height=cap_h)
    mc = mk.MerkleOpeningCircuit(a.leaf_len, height, cap_h, a.paths)
    gp, fp = sipp_amd.PlonkParams(80, 8, 2), mk.fri_params(mc.log_n)
    gc = sipp_amd.PlonkCircuit.from_dict(mc.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(mc.log_n, C.byref(gp), C.byref(fp), C.byref(gc))
    ctx = sipp_amd.Ctx(workspace_bytes=ws)
    _or, dcap, _keep = ctx.commit_ex(to_device(cols), log_n_tree, 1, cap_h)
    assert (dcap == b.cap).all()
    pr = mk.MerkleOpeningProver(ctx, a.leaf_len, height, cap_h, a.paths, fri=fp, params=gp)
    idx = [int(x) for x in rng.integers(0, 1 << a.log_leaves, size=a.paths)]
    leaves, sib = mr.opening(b, idx, height)
    pis = mc.public_inputs(dcap, idx, leaves)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    cs = mc.constants_sigmas()
    d_w, d_k = to_device(mc.partial_witness(dcap, idx, leaves, sib)), to_device(cs[:4])
    sched = sipp_amd.PlonkSchedule.from_dict(mc.schedule())
    gens = mc.generators()
    wit, prove, verify = [], [], []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        ctx.plonk_generate_witness_levels(d_w, d_k, mc.log_n, gens, pih, sched)
        wit.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pf = pr.prove(dcap, idx, leaves, sib)
        prove.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ok = pr.verify(pf)
        verify.append(time.perf_counter() - t0)
        assert ok == (0, 0), ok
    ms = lambda v: round(1e3 * min(v[1:]), 3)
    print(json.dumps({"paths": a.paths, "height": height, "leaf_len": a.leaf_len, "cap_height": cap_h, "log_n": mc.log_n, "rows_used": mc.rows_used,
                      "levels": mc.n_levels, "public_inputs": mc.n_pi, "witness_ms": ms(wit), "prove_ms": ms(prove), "verify_ms": ms(verify),
                      "prove_plus_verify_ms": round(ms(prove) + ms(verify), 3), "proof_words": int(len(pf))}))
    pr.close()
    ctx.close()


if __name__ == "__main__":
    main()
