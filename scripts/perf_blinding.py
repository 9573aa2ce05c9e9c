#!/usr/bin/env python3
"""Times of zero-knowledge blinding (sipp_amd/csrc/blind.hip) on one GPU, in a circuit of two gates without constraints (136 wires, 80
routed, identity permutation, 2 challenges, quotient degree factor 8, FRI rate_bits 3 / cap 4 / 28 queries / arity 16): the whole proof
without and with blinding (salted wires, Z / partial-products and quotient oracles: "SIPPPLK5"), the salt launch alone from the
per-kernel profile of the blinded proof, and the witness levels without and with the blinding rows -- the rows of the second gate, as
many as sipp_amd.circuit.blinding_counts asks for, filled by SIPP_GEN_RANDOM.  Prints one JSON line.
usage: perf_blinding.py [log2 rows = 18] [steps = 5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sipp_amd  # noqa: E402
from sipp_amd._lib import to_device  # noqa: E402
from sipp_amd.circuit import GEN_RANDOM, P, _gl_mul, _powers, _root_of_unity, blinding_counts  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << log_n
W, R, D, CH, K = 136, 80, 8, 2, 1
rng = np.random.default_rng(2026)
fp = sipp_amd.FriParams()
fp.rate_bits, fp.cap_height, fp.pow_bits, fp.num_queries, fp.pow_rule, fp.hiding = 3, 4, 16, 28, 0, 0
sipp_amd.lib().sipp_fri_const_arity(C.byref(fp), 4, 5, log_n)
fp_zk = sipp_amd.FriParams.from_buffer_copy(fp)
fp_zk.hiding = 1
regular, z = blinding_counts(fp, log_n)
blind_rows = min(regular + 2 * z, n // 2)
consts = np.zeros((K, n), dtype=np.uint64)
consts[0, n - blind_rows:] = 1                      # gate 1: the blinding rows, behind the circuit's
wires = rng.integers(0, P, size=(W, n), dtype=np.uint64)
pw = _powers(_root_of_unity(log_n), n)
sig = np.stack([_gl_mul(np.uint64(pow(7, j, P)), pw) for j in range(R)])
cs = np.concatenate([consts, sig])
circ = sipp_amd.PlonkCircuit.from_dict({"num_wires": W, "num_constants": K, "num_selectors": 1, "gates": [(0, 0, 0, 2, 0, 0), (0, 1, 0, 2, 0, 0)],
                                        "programs": np.zeros(0, dtype=np.int64)})
gp = sipp_amd.PlonkParams(R, D, CH)
digest, none = (1, 2, 3, 4), (0,) * 8
blind = sipp_amd.Blinding.of((5, 6, 7, 8), 0)
gens = [(GEN_RANDOM, 0, 1, 0, W, 0, 0, 0)]
sched = sipp_amd.PlonkSchedule.from_dict({"n_levels": 1, "rows": np.arange(n, dtype=np.uint32), "level_offsets": np.array([0, n], dtype=np.uint32),
                                          "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64),
                                          "copy_offsets": np.array([0, 0], dtype=np.uint32)})
cols = W + CH * (-(-R // D)) + CH * D + 12
ctx = sipp_amd.Ctx(workspace_bytes=int(8 * n * (9 * (K + R + cols) + 64) + (4 << 30)))


def timed(fn):
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / steps


try:
    d_w, d_cs = to_device(wires), to_device(cs)
    d_k = d_cs[:K]
    cs_or, cs_cap, keep = ctx.commit_ex(d_cs, log_n, fp.rate_bits, fp.cap_height)
    out = {"log_n": log_n, "steps": steps, "blinding_rows": int(blind_rows), "regular": int(regular), "z_pairs": int(z)}
    out["witness_levels_without_ms"] = timed(lambda: ctx.plonk_generate_witness_levels(d_w, d_k, log_n, [], None, sched))
    out["witness_levels_with_ms"] = timed(lambda: ctx.plonk_generate_witness_levels(d_w, d_k, log_n, gens, None, sched, blind=blind))
    out["prove_without_ms"] = timed(lambda: ctx.plonk_prove_gates_zk(d_w, d_cs, log_n, gp, fp, circ, digest, [], none, None, cs_oracle=cs_or))
    out["prove_with_ms"] = timed(lambda: ctx.plonk_prove_gates_zk(d_w, d_cs, log_n, gp, fp_zk, circ, digest, [], none, blind, cs_oracle=cs_or))
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(steps):
        proof = ctx.plonk_prove_gates_zk(d_w, d_cs, log_n, gp, fp_zk, circ, digest, [], none, blind, cs_oracle=cs_or)
    ctx.sync()
    rep = {k: round(v["ms"] / steps, 3) for k, v in ctx.profile_report().items()}
    ctx.profile(False)
    out["salt_launch_ms"] = rep.get("blind_salt")
    out["kernel_ms_per_proof"] = dict(sorted(rep.items(), key=lambda kv: -kv[1]))
    out["proof_words"] = int(len(proof))
    out["verified"] = sipp_amd.plonk_verify_gates_lookup(proof, cs_cap, gp, fp_zk, circ, digest, none) == 0
    print(json.dumps(out))
finally:
    ctx.close()
