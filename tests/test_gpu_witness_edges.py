"""The witness generators on the device at their value and layout edges: every entry of tests/_witness_edges.py through every launch path
that takes it -- sipp_plonk_generate_witness (one lane per row), and sipp_plonk_generate_witness_levels with thin levels on
plonk_witness_level_coop_kernel or plonk_witness_level_coop_rows_kernel and a level of 16384 rows on plonk_witness_level_kernel -- cell
for cell against the catalogue's exact reference (tests/test_oracle_witness_edges.py holds that reference against the CPU readings).  The
crafted Poseidon rows make the carry of every output of the first MDS layer fire in both of witness.hip's copies of that layer: mds(),
which one lane walks, and poseidon_lanes(), which both sixteen-lane kernels call."""
import numpy as np
import pytest

from tests import _witness_edges as we
from tests._device import NO_GRAPH, dev, host

pytestmark = pytest.mark.gpu

CASES = we.cases()


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def untouched_mismatch(e, got):
    """None, or the first cell no generator and no copy writes (rows of other selector values, gap cells, inputs) that came back changed"""
    bad = np.argwhere((got != e["wires"]) & ~e["written"])
    if bad.size == 0:
        return None
    j, r = int(bad[0][0]), int(bad[0][1])
    return "%s: wire %d row %d (%s) is no generator's, held %#x, came back %#x; %d such cells" % (
        e["name"], j, r, we.FAMILY[int(e["kind"][r])], int(e["wires"][j, r]), int(got[j, r]), len(bad))


@pytest.mark.parametrize("name,path", CASES, ids=["%s-%s" % c for c in CASES])
def test_device_witness_equals_the_reference_cell_for_cell(ctx, name, path):
    import sipp_amd
    e = we.entry(name)
    gens, sc = we.plan(e, path)
    L = sipp_amd.lib()
    d_c = dev(e["consts"])
    sched = sipp_amd.PlonkSchedule.from_dict(sc) if sc is not None else None
    # one entry also launch by launch (SIPP_ROUTE_WITNESS_NO_GRAPH), then the captured graph and its replay
    routes = (NO_GRAPH, 0, 0) if name == we.NO_GRAPH_ENTRY else (0,)
    try:
        for route in routes:
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            d_w = dev(e["wires"])
            if sched is None:
                ctx.plonk_generate_witness(d_w, d_c, e["log_n"], gens, e["pih"])
            else:
                ctx.plonk_generate_witness_levels(d_w, d_c, e["log_n"], gens, e["pih"], sched)
            ctx.sync()
            got = host(d_w)
            bad = we.first_mismatch(e, got)
            assert bad is None, "%s route %d: %s" % (path, route, bad)
            bad = untouched_mismatch(e, got)
            assert bad is None, "%s route %d: %s" % (path, route, bad)
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0
