#!/usr/bin/env python3
"""Both halves of plonky2's verify through the outer prover (sipp_amd/plonk_vanishing.py PlonkProofVerifier) for an inner proof of the
Poseidon kind at recursion-shaped parameters: the inner circuit is MerkleOpeningCircuit(16, 9, 4, 28) proved with
sipp_amd.circuit.fri_params (blowup 8, cap height 4, arity 16, `queries` queries, 16 bits of proof of work).  The vanishing circuit is
taken in its four VARIANTS in one interleaved run: today's (every inner gate from its monomials), the inner Poseidon gate through MDS
rows (poseidon_mds), the closing Horner in chunks of 8 (alpha_chunk), and both.  Beside the pair stands the ONE-circuit verifier
(sipp_amd/plonk_verifier.py PlonkVerifierCircuit, with poseidon_mds and alpha_chunk = 8: 17 generators), in the same interleaved runs:
its witness generation, PlonkVerifierProver.prove_proof and verify.  Run by hand.  Every GPU step is a child process under
its own `timeout`, the steps are chained, and nothing starts after a failure:

    inner     the device's inner proof; kept in a work file with its constants_sigmas cap and digest
    witness   witness generation alone (sipp_plonk_generate_witness_levels) of every variant's vanishing circuit and of the FRI
              circuit, interleaved
    prove     per variant PlonkProofVerifier.prove_proof's two proofs and their verification, the variants interleaved in one run; and
              for today's vanishing circuit sipp_circuit_prove_words against sipp_circuit_prove_inputs, interleaved

Prints one JSON line per step: the shapes (rows, levels, public and witness inputs of the circuits), then best, median and spread
(max - min) of `reps`.  One variant may be called faster than another, and prove_words faster than prove_inputs, only where the
difference exceeds the spread of their repeats.  Needs the oracle for the Merkle tree and the public-input hash (tests/_oracle.py;
built by build())."""
import argparse
import ctypes as C
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INNER_SHAPE = (16, 9, 4, 28)                                        # MerkleOpeningCircuit: leaf_len, height, cap_height, n_paths
INNER_DIGEST = (21, 22, 23, 24)
LIMITS = {"inner": 600, "witness": 600, "prove": 600}               # seconds, per step
VARIANTS = {"monomials": {}, "mds": {"poseidon_mds": True}, "chunks": {"alpha_chunk": 8}, "mds_chunks": {"poseidon_mds": True, "alpha_chunk": 8}}


def stats(v):
    v = v[1:]                                                       # the first repeat warms up
    return {"best_ms": round(1e3 * min(v), 3), "median_ms": round(1e3 * float(np.median(v)), 3), "spread_ms": round(1e3 * (max(v) - min(v)), 3)}


def ctx_for(log_n, gp, f, circuit):
    import sipp_amd
    gc = sipp_amd.PlonkCircuit.from_dict(circuit)
    return sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(log_n, C.byref(gp), C.byref(f), C.byref(gc)))


def inner_fri(a, log_n):
    from sipp_amd import circuit as ci
    return ci.fri_params(log_n, num_queries=a.queries)


def inner(a):
    import sipp_amd
    from oracle.py import plonky2_generic as g2
    from sipp_amd import circuit as ci
    from sipp_amd import merkle as mk
    leaf_len, height, cap_height, n_paths = INNER_SHAPE
    circ = mk.MerkleOpeningCircuit(*INNER_SHAPE)
    rng = np.random.default_rng(17)
    leaves = [[int(v) for v in row] for row in rng.integers(0, 1 << 62, size=(1 << (height + cap_height), leaf_len))]
    tree = g2.MerkleTree(leaves, cap_height)
    idx = [int(v) for v in rng.integers(0, len(leaves), size=n_paths)]
    args = ([v for d in tree.cap for v in d], idx, [v for i in idx for v in leaves[i]], [tree.prove(i) for i in idx])
    gp, f = sipp_amd.PlonkParams(80, 8, 2), inner_fri(a, circ.log_n)
    ctx = ctx_for(circ.log_n, gp, f, circ.circuit())
    pr = ci.CircuitProver(ctx, circ, fri=f, params=gp, digest=INNER_DIGEST)
    t0 = time.perf_counter()
    proof = pr.prove(*args)
    t_prove = time.perf_counter() - t0
    assert pr.verify(proof) == (0, 0)
    pickle.dump({"proof": np.asarray(proof, dtype=np.uint64), "cap": np.asarray(pr.cap), "log_n": circ.log_n, "circuit": circ.circuit(),
                 "n_pi": circ.n_pi}, open(a.work, "wb"))
    print(json.dumps({"step": "inner", "inner_log_n": circ.log_n, "inner_proof_words": int(len(proof)), "inner_prove_ms": round(1e3 * t_prove, 3)}))
    pr.close()
    ctx.close()


def circuits_of(a):
    from sipp_amd import plonk_vanishing as pv
    o = pickle.load(open(a.work, "rb"))
    vcs, fc = {}, None
    for name, kw in VARIANTS.items():
        ver = pv.PlonkProofVerifier(None, o["log_n"], (80, 8, 2), o["circuit"], inner_fri(a, o["log_n"]), o["n_pi"], fri=(0, 0),
                                    verifier_data=[(0, (0,) * 4)] * 2, **kw)
        vcs[name], fc = ver.vc, ver.fc
    return o, vcs, fc


JOINED = {"poseidon_mds": True, "alpha_chunk": 8}                   # the one-circuit verifier's variant: the one that fits the small table


def joined_shape(a, o):
    return (o["log_n"], (80, 8, 2), o["circuit"], inner_fri(a, o["log_n"]), o["n_pi"])


def describe(a):
    from sipp_amd import plonk_verifier as pj
    o, vcs, fc = circuits_of(a)
    jc = pj.PlonkVerifierCircuit(*joined_shape(a, o), **JOINED)
    line = {"step": "shape"}
    for name, c in [("vanishing_" + v, vc) for v, vc in vcs.items()] + [("fri_proof", fc), ("verifier_joined", jc)]:
        line[name] = {"rows_used": c.rows_used, "log_n": c.log_n, "levels": c.n_levels, "public_inputs": c.n_pi, "witness_inputs": len(c.in_cycle)}
    line["verifier_joined"]["generators"] = len(jc.generators())
    for v, vc in vcs.items():
        line["vanishing_" + v].update({"arithmetic_ops": vc.ops.count, "arithmetic_rows": len(vc.ops.rows), "mds_rows": len(vc.mds_rows),
                                       "ops_per_inner_gate": vc.gate_ops})
    print(json.dumps(line))


def arguments(o, vc, fc):
    """the argument tuples of both circuits from the inner proof, the transcript by the library's host permutation"""
    from sipp_amd import fri_proof as fp
    from sipp_amd import plonk_vanishing as pv
    v_args = pv.flat_proof_arguments(vc, o["proof"], INNER_DIGEST)
    t = vc.transcript(*v_args[:3])
    at = pv.HEADER_WORDS
    caps = [o["cap"].reshape(-1)] + [o["proof"][at + 4 * vc.n_cap * k:at + 4 * vc.n_cap * (k + 1)] for k in range(3)]
    section = o["proof"][at + 12 * vc.n_cap:len(o["proof"]) - vc.n_pi_inner]
    return v_args, fp.flat_proof_arguments(fc, section, caps, [t["zeta"], t["gzeta"]], (t["state"], []))


def witness(a):
    import sipp_amd
    from sipp_amd._lib import to_device
    from tests import _oracle
    from sipp_amd import plonk_verifier as pj
    o, vcs, fc = circuits_of(a)
    v_args, f_args = arguments(o, vcs["monomials"], fc)             # the arguments do not depend on the variant
    jc = pj.PlonkVerifierCircuit(*joined_shape(a, o), **JOINED)
    j_args = pj.flat_proof_arguments(jc, o["proof"], o["cap"], INNER_DIGEST)
    ctx = sipp_amd.Ctx(workspace_bytes=2 << 30)
    runs = {}
    for name, c, args, n_pub in ([("vanishing_" + v, vc, v_args, 4) for v, vc in vcs.items()] + [("fri_proof", fc, f_args, 6)] +
                                 [("verifier_joined", jc, j_args, 3)]):
        pih = _oracle.hash_no_pad(np.array(c.public_inputs(*args[:n_pub]), dtype=np.uint64))
        runs[name] = (c, to_device(c.partial_witness(*args)), to_device(c.constants_sigmas()[:c.num_constants]),
                      sipp_amd.PlonkSchedule.from_dict(c.schedule()), pih)
    wit = {name: [] for name in runs}
    for _ in range(a.reps + 1):
        for name, (c, d_w, d_k, sched, pih) in runs.items():       # interleaved: every circuit sees the same clocks
            ctx.plonk_generate_witness_levels(d_w, d_k, c.log_n, c.generators(), pih, sched)       # captures this circuit's graph
            t0 = time.perf_counter()
            ctx.plonk_generate_witness_levels(d_w, d_k, c.log_n, c.generators(), pih, sched)
            wit[name].append(time.perf_counter() - t0)
    print(json.dumps({"step": "witness", **{"witness_" + name: stats(v) for name, v in wit.items()}}))
    ctx.close()


def prove(a):
    import sipp_amd
    from sipp_amd import circuit as ci
    from sipp_amd import plonk_vanishing as pv
    from sipp_amd import plonk_verifier as pj
    o, vcs, fc = circuits_of(a)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    ctxs, vers = [], {}
    jc = pj.PlonkVerifierCircuit(*joined_shape(a, o), **JOINED)     # built here for its size alone; the prover builds its own
    j_fri = ci.fri_params(jc.log_n)
    ctxs.append(ctx_for(jc.log_n, gp, j_fri, jc.circuit()))
    joined = pj.PlonkVerifierProver(ctxs[0], *joined_shape(a, o), fri=j_fri, params=gp, **JOINED)
    for v, vc in vcs.items():                                       # one verifier per variant, each with its own two ctxs
        fris = (ci.fri_params(vc.log_n), ci.fri_params(fc.log_n))
        pair_ctxs = [ctx_for(c.log_n, gp, f, c.circuit()) for c, f in zip((vc, fc), fris)]
        ctxs += pair_ctxs
        vers[v] = pv.PlonkProofVerifier(pair_ctxs[0], o["log_n"], (80, 8, 2), o["circuit"], inner_fri(a, o["log_n"]), o["n_pi"],
                                        fri_ctx=pair_ctxs[1], fri=fris, outer_params=gp, **VARIANTS[v])
    van = vers["monomials"].vanishing
    v_args, _ = arguments(o, vcs["monomials"], fc)
    cells, values = van.circ.input_cells(*v_args)
    pis = van.circ.public_inputs(*v_args)
    t = {k: [] for k in [x + "_" + v for v in vers for x in ("prove_pair", "verify_pair")] + ["prove_words", "prove_inputs", "prove_joined",
                                                                                              "verify_joined"]}
    words = {}
    inner_pis = [int(x) for x in o["proof"][len(o["proof"]) - o["n_pi"]:]]
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()                                    # the one circuit, in the same round as the pairs
        one = joined.prove_proof(o["proof"], o["cap"], INNER_DIGEST)
        t["prove_joined"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = joined.verify(one, o["cap"], INNER_DIGEST)
        t["verify_joined"].append(time.perf_counter() - t0)
        assert got == inner_pis
        words["joined"] = int(len(one))
        for v, ver in vers.items():                                 # interleaved: every variant sees the same clocks
            t0 = time.perf_counter()
            pair = ver.prove_proof(o["proof"], o["cap"], INNER_DIGEST)
            t["prove_pair_" + v].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            got = ver.verify(pair, o["cap"], INNER_DIGEST)
            t["verify_pair_" + v].append(time.perf_counter() - t0)
            assert got == [int(x) for x in o["proof"][len(o["proof"]) - o["n_pi"]:]]
            words[v] = [int(len(p)) for p in pair]
        # the two entry points on the vanishing circuit, interleaved: both see the same clocks
        t0 = time.perf_counter()
        pf_w = van.prove_proof(o["proof"], INNER_DIGEST)
        t["prove_words"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pf_i = van.data.prove_inputs(cells, values, pis)
        t["prove_inputs"].append(time.perf_counter() - t0)
        assert (pf_w == pf_i).all()
    print(json.dumps({"step": "prove", **{k: stats(v) for k, v in t.items()}, "proof_words": words}))
    for ver in list(vers.values()) + [joined]:
        ver.close()
    for ctx in ctxs:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step", choices=["inner", "witness", "prove"], help="run one step in this process (what the parent starts)")
    ap.add_argument("--work", help="the work file between the steps")
    a = ap.parse_args()
    if a.step:
        return {"inner": inner, "witness": witness, "prove": prove}[a.step](a)
    with tempfile.TemporaryDirectory() as tmp:
        a.work = os.path.join(tmp, "inner.pickle")
        common = [sys.executable, os.path.abspath(__file__), "--queries", str(a.queries), "--reps", str(a.reps), "--work", a.work]
        for step in ("inner", "witness", "prove"):
            # a step that faults, aborts or runs out of time ends the run: nothing more is started on the card
            subprocess.check_call(["timeout", "-k", "10", str(LIMITS[step])] + common + ["--step", step])
            if step == "inner":
                describe(a)


if __name__ == "__main__":
    main()
