"""The one-circuit verifier on the device (sipp_amd/plonk_verifier.py), for the cases of tests/test_plonk_verifier_circuit.py: inner
proofs made by the device, equal to the oracle's; the device witness under every launch route against the Python reading cell for cell;
prove(*arguments) word for word the oracle's proof of the read witness and prove_proof (the input cells gathered on the device from the
inner proof's words) the same words, twice; both verifiers accept and verify returns the inner public inputs; tampered inner proofs
give outer proofs both verifiers refuse, the prover going on; a second inner proof verifies with its own public inputs.  The Poseidon
case with poseidon_mds is the circuit of 17 generators: the level kernels' wide argument struct (include/sipp_hip.h)."""
import ctypes as C

import pytest

from sipp_amd import circuit as ci
from sipp_amd import plonk_verifier as pj
from tests import _oracle
from tests import _plonk_vanishing_cases as cases
from tests import test_plonk_verifier_circuit as cpu
from tests._device import INTERP_ONE_LANE, NO_GRAPH, REDUCE_ONE_LANE, dev, first_mismatch, host
from tests.test_gpu_fri_generic import to_params
from tests.test_plonk_vanishing_circuit import TAMPERS

pytestmark = pytest.mark.gpu

DIGEST, OUTER = cpu.DIGEST, cpu.OUTER


def _ctx(log_n, params, gfp, circuit):
    import sipp_amd
    gp = sipp_amd.PlonkParams(*params)
    gc = sipp_amd.PlonkCircuit.from_dict(circuit)
    return sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(log_n, C.byref(gp), C.byref(gfp), C.byref(gc)))


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)
    yield c
    c.close()


def _case(case):
    """per case: the inner proof by the DEVICE, the joined circuit's prover, the arguments; closes everything afterwards"""
    import sipp_amd
    b = cpu.build(case)
    o, c = b["o"], b["c"]
    gfp = to_params(o["ofp"])
    ic = _ctx(o["c"].log_n, o["params"], gfp, o["circ"])
    inner = ci.CircuitProver(ic, o["c"], fri=gfp, params=sipp_amd.PlonkParams(*o["params"]), digest=cases.INNER_DIGEST)
    proof = inner.data.prove(o["pw"], o["pis"])
    assert inner.verify(proof) == (0, 0) and (inner.cap == o["cap"]).all()
    ofp = cpu.outer_fri(c)
    oc = _ctx(c.log_n, (80, 8, 2), to_params(ofp), c.circuit())
    pr = pj.PlonkVerifierProver(oc, *cpu.shape(o), fri=to_params(ofp), digest=DIGEST, **b["kw"])
    assert pr.circ.log_n == c.log_n and pr.circ.generators() == c.generators()
    yield {"b": b, "o": o, "c": c, "inner": inner, "proof": proof, "pr": pr, "ofp": ofp}
    pr.close()
    inner.close()
    for x in (oc, ic):
        x.close()


# the 2^13 table of the Poseidon case without its MDS rows stays with the CPU file
GPU_CASES = ("basic", "ragged", "poseidon-mds")


@pytest.fixture(scope="module", params=GPU_CASES)
def whole(request):
    yield from _case(request.param)


@pytest.fixture(scope="module")
def ragged():
    yield from _case("ragged")


def test_the_device_makes_the_oracles_inner_proof(whole):
    want = whole["b"]["proof"]
    assert len(whole["proof"]) == len(want) and (whole["proof"] == want).all()


def test_the_device_witness_is_the_reading_on_every_route(ctx, whole):
    import sipp_amd
    b, c, L = whole["b"], whole["c"], sipp_amd.lib()
    want, pis, pih = cpu.witness(b)
    pw = c.partial_witness(*b["args"])
    sched = sipp_amd.PlonkSchedule.from_dict(c.schedule())
    d_c = dev(b["cs"][:c.num_constants])
    try:
        for route in (0, NO_GRAPH, INTERP_ONE_LANE, REDUCE_ONE_LANE):
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            d_w = dev(pw)
            ctx.plonk_generate_witness_levels(d_w, d_c, c.log_n, c.generators(), pih, sched)
            assert first_mismatch(host(d_w), want) is None, route
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_the_outer_proof_is_the_oracles_and_proves_from_the_inner_proofs_words(whole):
    b, c, o, pr = whole["b"], whole["c"], whole["o"], whole["pr"]
    ref, cap = cpu.outer_proof(b)
    assert (pr.cap == cap).all()
    pf = pr.prove(*b["args"])
    assert len(pf) == len(ref) and (pf == ref).all()
    assert pr.verify(pf) == (0, 0) and _oracle.plonk_verify_gates(pf, pr.cap, OUTER, whole["ofp"], pr.circuit, DIGEST) == 0
    for _ in range(2):
        words = pr.prove_proof(whole["proof"], o["cap"], cases.INNER_DIGEST)
        assert len(words) == len(pf) and (words == pf).all()
    assert pr.verify(pf, o["cap"], cases.INNER_DIGEST) == o["pis"]


@pytest.mark.parametrize("what", TAMPERS + tuple(sorted(cpu.SECTION_TAMPERS)))
def test_tampered_inner_proofs_are_refused_and_the_prover_goes_on(ragged, what):
    b, o, pr = ragged["b"], ragged["o"], ragged["pr"]
    pf, digest = cpu.tampered_proof(b, what)
    bad = pr.prove_proof(pf, o["cap"], digest)
    assert pr.verify(bad)[0] != 0 and _oracle.plonk_verify_gates(bad, pr.cap, OUTER, ragged["ofp"], pr.circuit, DIGEST) != 0
    with pytest.raises(ValueError, match="refused"):
        pr.verify(bad, o["cap"], digest)
    assert pr.verify(pr.prove_proof(ragged["proof"], o["cap"], cases.INNER_DIGEST), o["cap"], cases.INNER_DIGEST) == o["pis"]


def test_a_second_inner_proof_verifies_with_its_own_public_inputs(whole):
    o, pr = whole["o"], whole["pr"]
    pis, pw = cpu.second_inner_inputs(o)
    other = whole["inner"].data.prove(pw, pis)
    assert whole["inner"].verify(other) == (0, 0) and pis != o["pis"]
    assert pr.verify(pr.prove_proof(other, o["cap"], cases.INNER_DIGEST), o["cap"], cases.INNER_DIGEST) == pis
