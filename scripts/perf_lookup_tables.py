#!/usr/bin/env python3
"""scripts/perf_lookups.py's shape with TWO tagged tables (description word 7): the 2^16 entries are split into two dense tables of 2^15
(tag 0: t -> 0, a range table; tag 1: t -> 3 t mod 65521), table rows of 8 slots, every other row a looking row of 16 pairs whose
tag alternates row by row, in a circuit of one gate without constraints (136 wires, 80 routed, identity permutation, 2 challenges,
quotient degree factor 8, FRI rate_bits 3 / cap 4 / 28 queries).  The same lines as perf_lookups.py -- the multiplicities (with the
host-side index build), the S / U columns, the proof with and without the description, the per-kernel profile -- and the time of
witness generation when every looking row is a FUNCTION row: SIPP_GEN_LOOKUP fills all 16 y cells of every looking row from its x
cells, on sipp_plonk_generate_witness (one launch over all rows) and on sipp_plonk_generate_witness_levels (one level of the looking
rows, through the captured graph).  Prints one JSON line.
usage: perf_lookup_tables.py [log2 rows = 18] [steps = 5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sipp_amd  # noqa: E402
from sipp_amd._lib import to_device  # noqa: E402
from sipp_amd.circuit import GEN_LOOKUP, _gl_mul, _powers, _root_of_unity, P  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 18
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << log_n
W, R, D, CH, N_LOOK, N_TAB, BITS = 136, 80, 8, 2, 16, 8, 16
TAB0, TAG0 = 3, 3 + 2 * N_TAB                        # selector, q_look, q_tab, the table columns, the two tag columns, c0 = row0, c1 = T
BASE = TAG0 + 2
K = BASE + 2
desc = (1, 0, N_LOOK, 2, TAB0, 2 * N_LOOK, N_TAB, TAG0)
rng = np.random.default_rng(2026)
table_rows = min((1 << BITS) // N_TAB, n // 2)
half = table_rows // 2
T = half * N_TAB                                     # entries of either table
f = [np.zeros(T, dtype=np.uint64), (np.arange(T, dtype=np.uint64) * np.uint64(3)) % np.uint64(65521)]
consts = np.zeros((K, n), dtype=np.uint64)
consts[2, :table_rows] = 1
consts[1, table_rows:] = 1
for tag, row0 in ((0, 0), (1, half)):
    consts[TAG0 + 1, row0:row0 + half] = tag
    for k in range(N_TAB):
        consts[TAB0 + 2 * k, row0:row0 + half] = np.arange(half, dtype=np.uint64) * np.uint64(N_TAB) + np.uint64(k)
        consts[TAB0 + 2 * k + 1, row0:row0 + half] = f[tag][k::N_TAB]
look = np.arange(table_rows, n)
tags = (look & 1).astype(np.uint64)
consts[TAG0, look] = tags
consts[BASE, look] = tags * np.uint64(half)          # every looking row a function row: row0 and T of its table
consts[BASE + 1, look] = T
wires = rng.integers(0, P, size=(W, n), dtype=np.uint64)
for k in range(N_LOOK):
    x = rng.integers(0, T, size=len(look), dtype=np.uint64)
    wires[2 * k, look] = x
    wires[2 * k + 1, look] = np.where(tags == 1, f[1][x.astype(np.int64)], 0)
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
etas, thetas = [int(v) for v in rng.integers(1 << 40, P, size=CH, dtype=np.uint64)], [int(v) for v in rng.integers(1 << 40, P, size=CH, dtype=np.uint64)]
cols = W + CH * (-(-R // D)) + CH * (-(-N_LOOK // D) + -(-N_TAB // D)) + CH * D
ctx = sipp_amd.Ctx(workspace_bytes=int(8 * n * (9 * (K + R + cols) + 64) + (4 << 30)))
gens = [(GEN_LOOKUP, 0, 0, 0, N_LOOK, TAB0, N_TAB, BASE)]      # the one gate's selector value is 0: every row holds it, T = 0 off the looking rows
sched = sipp_amd.PlonkSchedule.from_dict({"n_levels": 1, "rows": look.astype(np.uint32), "level_offsets": np.array([0, len(look)], dtype=np.uint32),
                                          "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64),
                                          "copy_offsets": np.array([0, 0], dtype=np.uint32)})


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
    out = {"log_n": log_n, "steps": steps, "n_look": N_LOOK, "n_tab": N_TAB, "tables": 2, "table_entries": int(2 * T), "looking_rows": int(len(look))}
    # the generator first, from y cells it has to overwrite; what it leaves is what the argument below proves
    y_rows = np.arange(1, 2 * N_LOOK, 2)
    spoiled = wires.copy()
    spoiled[np.ix_(y_rows, look)] = 0xDEADBEEF
    d_w.copy_(to_device(spoiled))
    out["witness_row_local_ms"] = timed(lambda: ctx.plonk_generate_witness(d_w, d_k, log_n, gens))
    d_w.copy_(to_device(spoiled))
    out["witness_levels_ms"] = timed(lambda: ctx.plonk_generate_witness_levels(d_w, d_k, log_n, gens, None, sched))
    out["witness_is_the_table"] = bool((sipp_amd._lib.to_host(d_w) == wires).all())
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
