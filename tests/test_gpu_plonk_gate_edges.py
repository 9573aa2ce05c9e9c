"""sipp_plonk_prove_gates on the edge gate sets of tests/_gate_edges.py: the compiled quotient (compile_gates + plonk_quotient_kernel with
its chained pure powers, square-and-multiply, constant monomials, merged duplicates, the many_sel filter and the per-constraint alpha
offsets) must give the oracle's proof word for word, which every verifier then judges as it judges the oracle's; the same through
pre-committed oracles and through CircuitData over host arrays; the prover's own limits (circuit_check) on either side, with the ctx
still proving afterwards."""
import ctypes as C

import numpy as np
import pytest

from tests import _gate_edges as ge
from tests import _oracle
from tests._device import dev
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk_gate_edges import DIGEST, assert_verdicts, cs_cap

pytestmark = pytest.mark.gpu

ENTRIES = [f for _, f in ge.ENTRIES]
IDS = [name for name, _ in ge.ENTRIES]


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def oracle_proof(e, circ=None):
    return _oracle.plonk_prove_gates(e["wires"], e["cs"], e["log_n"], ge.params(e), ge.fri_params(e), circ or e["circ"], DIGEST, e["pis"])


def device_proof(ctx, e, circ=None, **kw):
    import sipp_amd
    gp = sipp_amd.PlonkParams(e["num_routed"], ge.MAX_DEGREE, e["num_challenges"])
    return ctx.plonk_prove_gates(dev(e["wires"]), dev(e["cs"]), e["log_n"], gp, to_params(ge.fri_params(e)),
                                 sipp_amd.PlonkCircuit.from_dict(circ or e["circ"]), DIGEST, e["pis"], **kw)


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_device_proof_is_the_oracles(ctx, make):
    """word for word the oracle's proof (a mismatch names its first word and section), judged by the oracle's verifier, verify.cpp and
    the Python replay as the oracle's proof is; with constants_sigmas and wires committed beforehand the same words come out"""
    e = make()
    ref = oracle_proof(e)
    got = device_proof(ctx, e)
    msg = ge.first_difference(got, ref, e)
    assert msg is None, msg
    assert_verdicts(got, e)
    rb, ch = ge.FRI["rate_bits"], ge.FRI["cap_height"]
    cs_or, cap, keep1 = ctx.commit_ex(dev(e["cs"]), e["log_n"], rb, ch)
    w_or, w_cap, keep2 = ctx.commit_ex(dev(e["wires"]), e["log_n"], rb, ch)
    assert (cap == cs_cap(e)).all()
    got2 = device_proof(ctx, e, wires_oracle=w_or, wires_cap=w_cap, cs_oracle=cs_or)
    msg = ge.first_difference(got2, ref, e)
    assert msg is None, "pre-committed: " + msg
    del keep1, keep2


@pytest.mark.parametrize("make", [ge.single_selector, lambda: ge.rich(C=8)], ids=["single_selector", "rich_C8"])
def test_circuit_data_over_host_arrays(make):
    """sipp_circuit_build / _prove / _verify with an explicit digest, no generators and the complete wire table: the oracle's proof,
    accepted by the data's own verify and the oracle's"""
    import sipp_amd
    e = make()
    gp = sipp_amd.PlonkParams(e["num_routed"], ge.MAX_DEGREE, e["num_challenges"])
    ofp = ge.fri_params(e)
    gfp, gc = to_params(ofp), sipp_amd.PlonkCircuit.from_dict(e["circ"])
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(e["log_n"], C.byref(gp), C.byref(gfp), C.byref(gc))
    c = sipp_amd.Ctx(workspace_bytes=ws)
    try:
        data = sipp_amd.CircuitData(c, e["log_n"], gp, gfp, gc, e["cs"], [], digest=DIGEST)
        assert (data.cap == cs_cap(e)).all() and [int(x) for x in data.digest] == list(DIGEST)
        pf = data.prove(e["wires"], e["pis"])
        msg = ge.first_difference(pf, oracle_proof(e), e)
        assert msg is None, msg
        assert data.verify(pf) == (0, 0)
        assert _oracle.plonk_verify_gates(pf, cs_cap(e), ge.params(e), ofp, e["circ"], DIGEST) == 0
        data.close()
    finally:
        c.close()


def raw_prove_rc(ctx, e, circ):
    """sipp_plonk_prove_gates called directly (the wrapper sizes its buffer with sipp_plonk_gates_proof_size, which refuses 4097 wires or
    1025 constants itself): tables of the circuit's own shape, zeros"""
    import sipp_amd
    n, R = 1 << e["log_n"], e["num_routed"]
    wires = dev(np.zeros((circ["num_wires"], n), dtype=np.uint64))
    cs = dev(np.zeros((circ["num_constants"] + R, n), dtype=np.uint64))
    gp = sipp_amd.PlonkParams(R, ge.MAX_DEGREE, e["num_challenges"])
    fp, gc = to_params(ge.fri_params(e)), sipp_amd.PlonkCircuit.from_dict(circ)
    cap = 1 << 20
    out, length = np.zeros(cap, dtype=np.uint64), C.c_size_t()
    pis = list(e["pis"])
    return ctx.L.sipp_plonk_prove_gates(ctx.h, wires.data_ptr(), cs.data_ptr(), None, None, None, e["log_n"], C.byref(gp), C.byref(fp), C.byref(gc),
                                        ctx._u64(DIGEST), ctx._u64(pis) if pis else None, len(pis), out.ctypes.data, cap, C.byref(length))


@pytest.mark.parametrize("limit", range(len(ge.LIMIT_IDS)), ids=ge.LIMIT_IDS)
def test_prover_limits(ctx, limit):
    """circuit_check inside sipp_plonk_prove_gates: just inside a limit the device proves the oracle's proof; one step beyond it the call
    is SIPP_E_BADARG before any kernel runs; the ctx proves again afterwards"""
    name, inside, outside, outside_entry = ge.limits()[limit]
    ref = oracle_proof(inside)
    msg = ge.first_difference(device_proof(ctx, inside), ref, inside)
    assert msg is None, msg
    assert raw_prove_rc(ctx, outside_entry or inside, outside) == -1, name
    msg = ge.first_difference(device_proof(ctx, inside), ref, inside)
    assert msg is None, "after the refusal: " + msg
