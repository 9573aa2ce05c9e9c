"""sipp_plonk_generate_witness_levels at and past sixteen generators, against the CPU replay of tests/_witness_reading.py, cell for cell.
The circuits are tests/_many_generators.py's (tests/test_many_generators_circuits.py holds them to what is said here): 16 generators, the
last circuit of the narrow argument struct; 17, 31 and 32, which take the wide instantiation of every level kernel, with a Poseidon-swap,
an interpolation, a Reducing and a ReducingExt generator at index 16 and behind it, each wide sixteen-lane kernel picked by one circuit
at least (plonk_witness_level_coop_kernel by a plain Poseidon generator without a swap); levels of 5, 3 and 1 rows; one level of 16384
rows in a 2^15 table (plonk_witness_level_kernel); every route.  33 generators are refused on the host, by code and message, with the
table untouched, and the same ctx then serves a circuit of 32; sipp_circuit_build refuses them too."""
import pytest

from tests import _many_generators as mg
from tests._device import INTERP_ONE_LANE, NO_GRAPH, REDUCE_ONE_LANE, dev, first_mismatch, host, run_levels

pytestmark = pytest.mark.gpu

ROUTES = (0, 0, NO_GRAPH, INTERP_ONE_LANE, REDUCE_ONE_LANE, INTERP_ONE_LANE | REDUCE_ONE_LANE | NO_GRAPH)


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 28)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(mg.CIRCUITS))
def test_thin_levels_on_every_route(ctx, name):
    c = mg.ManyGenerators(*mg.CIRCUITS[name])
    w, k = c.table(1601)
    want = run_levels(ctx, w, k, c.log_n, c.generators(), c.schedule(), ROUTES)
    assert (want != w).any(axis=0)[:c.rows_used].all()


@pytest.mark.parametrize("name", ["16", "17-swap-at-16", "32-spread"])
def test_a_level_of_16384_rows_on_every_route(ctx, name):
    c = mg.ManyGenerators(*mg.CIRCUITS[name], wide_level=True)
    sc = c.schedule()
    assert c.log_n == 15 and int(sc["level_offsets"][1]) == mg.WIDE_ROWS
    w, k = c.table(1602)
    run_levels(ctx, w, k, c.log_n, c.generators(), sc, ROUTES)


def test_33_generators_are_refused_on_the_host_and_the_ctx_serves_32_after(ctx):
    import sipp_amd
    c = mg.ManyGenerators(33, {16: "interp", 30: "reducing_ext", 32: "swap"})
    w, k = c.table(1603)
    d_w = dev(w)
    with pytest.raises(sipp_amd.SippError) as e:
        ctx.plonk_generate_witness_levels(d_w, dev(k), c.log_n, c.generators(), None, sipp_amd.PlonkSchedule.from_dict(c.schedule()))
    assert e.value.code == -1 and "more than 32 generators" in str(e.value)
    ctx.sync()
    assert first_mismatch(host(d_w), w) is None                 # nothing was launched
    good = mg.ManyGenerators(*mg.CIRCUITS["32"])
    w, k = good.table(1604)
    run_levels(ctx, w, k, good.log_n, good.generators(), good.schedule(), (0, NO_GRAPH))


def test_circuit_build_refuses_33_generators_with_a_schedule(ctx):
    import sipp_amd
    from sipp_amd import _lib
    from sipp_amd.circuit import fri_params
    c = mg.ManyGenerators(33, {32: "swap"})
    with pytest.raises(sipp_amd.SippError) as e:
        _lib.CircuitData(ctx, c.log_n, _lib.PlonkParams(c.num_routed, 8, 2), fri_params(c.log_n), _lib.PlonkCircuit.from_dict(c.circuit()),
                         c.constants_sigmas(), c.generators(), sched=c.schedule())
    assert e.value.code == -1 and "more than 32 generators" in str(e.value)
    good = mg.ManyGenerators(*mg.CIRCUITS["32"])                # the ctx is usable afterwards
    w, k = good.table(1605)
    run_levels(ctx, w, k, good.log_n, good.generators(), good.schedule(), (0,))
