#!/usr/bin/env python3
"""Times of the lookup argument (sipp_amd/csrc/lookup.hip) on one GPU: a 2^16-entry range table (v, 0) in table rows of 8 slots, every
other row a looking row of 16 pairs, in a circuit of one gate without constraints (136 wires, 80 routed, identity permutation,
2 challenges, quotient degree factor 8, FRI rate_bits 3 / cap 4 / 28 queries): the multiplicities (with the host-side index build of the
raw call), the S / U columns, and the whole proof with and without the description -- the difference is what the argument adds -- with
the per-kernel profile of the proof with lookups.  Prints one JSON line.
usage: perf_lookups.py [log2 rows = 18] [steps = 5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sipp_amd  # noqa: E402
from sipp_amd._lib import to_device  # noqa: E402
from sipp_amd.circuit import _gl_mul, _powers, _root_of_unity, P  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << log_n
W, R, D, CH, N_LOOK, N_TAB, BITS = 136, 80, 8, 2, 16, 8, 16
K = 3 + 2 * N_TAB                                   # selector, q_look, q_tab, the table columns
desc = (1, 0, N_LOOK, 2, 3, 2 * N_LOOK, N_TAB, 0)
rng = np.random.default_rng(2026)
table_rows = min((1 << BITS) // N_TAB, n // 2)
consts = np.zeros((K, n), dtype=np.uint64)
consts[2, :table_rows] = 1
consts[1, table_rows:] = 1
vals = np.arange(table_rows * N_TAB, dtype=np.uint64).reshape(table_rows, N_TAB)
for k in range(N_TAB):
    consts[3 + 2 * k, :table_rows] = vals[:, k]
wires = rng.integers(0, P, size=(W, n), dtype=np.uint64)
for k in range(N_LOOK):
    wires[2 * k, table_rows:] = rng.integers(0, table_rows * N_TAB, size=n - table_rows, dtype=np.uint64)
    wires[2 * k + 1, table_rows:] = 0
pw = _powers(_root_of_unity(log_n), n)
sig = np.stack([_gl_mul(np.uint64(pow(7, j, P)), pw) for j in range(R)])
cs = np.concatenate([consts, sig])
circ = sipp_amd.PlonkCircuit.from_dict({"num_wires": W, "num_constants": K, "num_selectors": 1, "gates": [(0, 0, 0, 1, 0, 0)],
                                        "programs": np.zeros(0, dtype=np.int64)})
gp = sipp_amd.PlonkParams(R, D, CH)
fp = sipp_amd.FriParams()
fp.rate_bits, fp.cap_height, fp.pow_bits, fp.num_queries, fp.pow_rule, fp.hiding = 3, 4, 16, 28, 0, 0
sipp_amd.lib().sipp_fri_const_arity(C.byref(fp), 4, 5, log_n)
digest = (1, 2, 3, 4)
# challenges as the transcript would draw them (a small theta sits ON a table value: SIPP_E_WITNESS, rightly)
etas, thetas = [int(v) for v in rng.integers(1 << 40, P, size=CH, dtype=np.uint64)], [int(v) for v in rng.integers(1 << 40, P, size=CH, dtype=np.uint64)]
cols = W + CH * (-(-R // D)) + CH * (-(-N_LOOK // D) + -(-N_TAB // D)) + CH * D
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
    out = {"log_n": log_n, "steps": steps, "n_look": N_LOOK, "n_tab": N_TAB, "table_entries": int(table_rows * N_TAB), "looking_rows": int(n - table_rows)}
    out["multiplicities_with_index_build_ms"] = timed(lambda: ctx.plonk_lookup_multiplicities(d_w, d_k, log_n, 1, desc))
    out["sums_ms"] = timed(lambda: ctx.plonk_lookup_sums(d_w, d_k, log_n, 1, gp, desc, etas, thetas))
    out["prove_without_ms"] = timed(lambda: ctx.plonk_prove_gates(d_w, d_cs, log_n, gp, fp, circ, digest, [], cs_oracle=cs_or))
    out["prove_with_ms"] = timed(lambda: ctx.plonk_prove_gates_lookup(d_w, d_cs, log_n, gp, fp, circ, digest, [], desc, cs_oracle=cs_or))
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(steps):
        proof = ctx.plonk_prove_gates_lookup(d_w, d_cs, log_n, gp, fp, circ, digest, [], desc, cs_oracle=cs_or)
    ctx.sync()
    rep = {k: round(v["ms"] / steps, 3) for k, v in ctx.profile_report().items()}
    ctx.profile(False)
    out["kernel_ms_per_proof"] = dict(sorted(rep.items(), key=lambda kv: -kv[1]))
    out["proof_words"] = int(len(proof))
    out["verified"] = sipp_amd.plonk_verify_gates_lookup(proof, cs_cap, gp, fp, circ, digest, desc) == 0
    print(json.dumps(out))
finally:
    ctx.close()
