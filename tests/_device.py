"""What the GPU tests of the witness generators share: arrays to the device and back, the first differing cell, a level schedule as the
dictionary sipp_amd.PlonkSchedule.from_dict takes, and a schedule run under a sequence of kernel routes against the Python reading
(tests/_witness_reading.py).  A plain module: every test module keeps its own ctx fixture, since the workspace sizes differ."""
import numpy as np

# include/sipp_hip.h SIPP_ROUTE_WITNESS_*
NO_GRAPH, INTERP_ONE_LANE, REDUCE_ONE_LANE = 4, 16, 32


def dev(a):
    from sipp_amd._lib import to_device
    return to_device(a)


def host(t):
    from sipp_amd._lib import to_host
    return to_host(t)


def first_mismatch(got, want):
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else (int(bad[0][0]), int(bad[0][1]), len(bad))


def levels(level_rows, copies=None):
    """schedule dict from per-level row lists and, where outputs feed later levels, per-level (src, dst) cell lists"""
    copies = [[] for _ in level_rows] if copies is None else copies
    rows = np.concatenate([np.asarray(r, dtype=np.uint32) for r in level_rows])
    lo = np.cumsum([0] + [len(r) for r in level_rows]).astype(np.uint32)
    src = np.concatenate([np.asarray([s for s, _ in c], dtype=np.uint64) for c in copies]) if any(copies) else np.zeros(0, np.uint64)
    dst = np.concatenate([np.asarray([d for _, d in c], dtype=np.uint64) for c in copies]) if any(copies) else np.zeros(0, np.uint64)
    co = np.cumsum([0] + [len(c) for c in copies]).astype(np.uint32)
    return {"n_levels": len(level_rows), "rows": rows, "level_offsets": lo, "copy_src": src, "copy_dst": dst, "copy_offsets": co}


def run_levels(ctx, w, consts, log_n, gens, sc, routes):
    """sipp_plonk_generate_witness_levels under every route in turn (0: captured graph, then its replay), each time on a fresh copy of
    the table and against the CPU replay, which is returned"""
    import sipp_amd
    from tests import _witness_reading as rd
    want = rd.replay(w, consts, gens, None, sc)
    sched = sipp_amd.PlonkSchedule.from_dict(sc)
    L = sipp_amd.lib()
    d_c, d_w = dev(consts), dev(w)
    try:
        for route in routes:
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            d_w.copy_(dev(w))
            ctx.plonk_generate_witness_levels(d_w, d_c, log_n, gens, None, sched)
            assert first_mismatch(host(d_w), want) is None, route
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
    return want
