#!/usr/bin/env python3
"""Times of the outer proof under the two tree hashers (Poseidon; Keccak-256 truncated to 25 bytes, sipp_amd/csrc/keccak.hip) on one GPU,
in scripts/perf_blinding.py's circuit of two gates without constraints (136 wires, 80 routed, identity permutation, 2 challenges, quotient
degree factor 8, FRI rate_bits 3 / cap 4 / 28 queries / arity 16): per hasher the whole proof (its constants_sigmas oracle committed once,
with the same hasher), and from the per-kernel profile of `steps` proofs the leaf launches and the level launches.  The hashers alternate
(Poseidon, Keccak, Poseidon, ...: `rounds` of each) inside the one process, so that neither gets the warmer card.  Prints one JSON line.
usage: perf_keccak.py [log2 rows = 18] [steps = 5] [rounds = 3]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sipp_amd  # noqa: E402
from sipp_amd import _lib  # noqa: E402
from sipp_amd._lib import to_device  # noqa: E402
from sipp_amd.circuit import P, _gl_mul, _powers, _root_of_unity  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
n = 1 << log_n
W, R, D, CH, K = 136, 80, 8, 2, 1
rng = np.random.default_rng(2026)
fp = sipp_amd.FriParams()
fp.rate_bits, fp.cap_height, fp.pow_bits, fp.num_queries, fp.pow_rule, fp.hiding = 3, 4, 16, 28, 0, 0
sipp_amd.lib().sipp_fri_const_arity(C.byref(fp), 4, 5, log_n)
consts = np.zeros((K, n), dtype=np.uint64)
wires = rng.integers(0, P, size=(W, n), dtype=np.uint64)
pw = _powers(_root_of_unity(log_n), n)
sig = np.stack([_gl_mul(np.uint64(pow(7, j, P)), pw) for j in range(R)])
cs = np.concatenate([consts, sig])
circ = sipp_amd.PlonkCircuit.from_dict({"num_wires": W, "num_constants": K, "num_selectors": 1, "gates": [(0, 0, 0, 1, 0, 0)],
                                        "programs": np.zeros(0, dtype=np.int64)})
gp = sipp_amd.PlonkParams(R, D, CH)
digest = (1, 2, 3, 4)
cols = W + CH * (-(-R // D)) + CH * D
ctx = sipp_amd.Ctx(workspace_bytes=int(8 * n * (9 * (K + R + cols) + 64) + (4 << 30)))
LEAVES = {"poseidon": ("poseidon_leaves", "poseidon_leaves_pair", "poseidon_leaves_noop", "fri_leaves"),
          "keccak": ("keccak_leaves", "keccak_leaves_noop", "keccak_fri_leaves")}
LEVELS = {"poseidon": ("merkle_subtree",), "keccak": ("keccak_merkle_subtree",)}

try:
    d_w, d_cs = to_device(wires), to_device(cs)
    oracles = {h: ctx.commit_ex(d_cs, log_n, fp.rate_bits, fp.cap_height, hasher=h) for h in ("poseidon", "keccak")}

    def prove(h):
        return ctx.plonk_prove_gates_h(d_w, d_cs, log_n, gp, fp, circ, digest, [], None, None, h, cs_oracle=oracles[h][0])

    out = {"log_n": log_n, "steps": steps, "rounds": rounds}
    runs = {"poseidon": [], "keccak": []}
    for h in ("poseidon", "keccak"):
        prove(h)
    ctx.sync()
    for _ in range(rounds):
        for h in ("poseidon", "keccak"):
            t0 = time.perf_counter()
            for _ in range(steps):
                proof = prove(h)
            ctx.sync()
            runs[h].append(round(1e3 * (time.perf_counter() - t0) / steps, 3))
    for h in ("poseidon", "keccak"):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(steps):
            proof = prove(h)
        ctx.sync()
        rep = {k: round(v["ms"] / steps, 3) for k, v in ctx.profile_report().items()}
        ctx.profile(False)
        out[h] = {"prove_ms_runs": runs[h], "prove_ms_median": sorted(runs[h])[len(runs[h]) // 2],
                  "leaf_launches_ms": round(sum(rep.get(k, 0.0) for k in LEAVES[h]), 3),
                  "level_launches_ms": round(sum(rep.get(k, 0.0) for k in LEVELS[h]), 3),
                  "kernel_ms_per_proof": dict(sorted(rep.items(), key=lambda kv: -kv[1])[:8]),
                  "proof_words": int(len(proof)),
                  "verified": _lib.plonk_verify_gates_h(proof, oracles[h][1], gp, fp, circ, digest, None, h) == 0}
    print(json.dumps(out))
finally:
    ctx.close()
