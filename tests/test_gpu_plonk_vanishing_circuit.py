"""The vanishing circuit on the device (sipp_amd/plonk_vanishing.py): inner proofs made by the device for the three inner circuits of
tests/_plonk_vanishing_cases.py; the device witness under every launch route against the Python reading (tests/_witness_reading.py)
cell for cell; the outer proof word for word the oracle's of the read witness, accepted by both verifiers; prove_proof (the input cells
gathered on the device from the inner proof's words) against prove(*arguments); tampered inner proofs refused, the prover going on; the
pair of PlonkProofVerifier accepted with the inner public inputs, a stitched pair refused."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import circuit as ci
from sipp_amd import plonk_vanishing as pv
from tests import _challenger_reading  # noqa: F401  (registers the reading of generator kind 15)
from tests import _oracle
from tests import _plonk_vanishing_cases as cases
from tests import _witness_reading as rd
from tests._device import INTERP_ONE_LANE, NO_GRAPH, REDUCE_ONE_LANE, dev, first_mismatch, host
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri
from tests.test_plonk_vanishing_circuit import TAMPERS, read, tampered

pytestmark = pytest.mark.gpu

DIGEST = (89, 90, 91, 92)
OUTER = _oracle.plonk_params(80, 8, 2)


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


def _inner_prover(o):
    import sipp_amd
    gfp = to_params(o["ofp"])
    c = _ctx(o["c"].log_n, o["params"], gfp, o["circ"])
    return ci.CircuitProver(c, o["c"], fri=gfp, params=sipp_amd.PlonkParams(*o["params"]), digest=cases.INNER_DIGEST), c


FRI_LOG_N = 11                                                  # of the FRI circuit, for every case


def _case(name):
    """per inner circuit: its proof by the DEVICE, the verifier pair built for it, the arguments; closes everything afterwards"""
    o = cases.inner(name)
    inner, ic = _inner_prover(o)
    proof = inner.data.prove(o["pw"], o["pis"])
    assert inner.verify(proof) == (0, 0) and (inner.cap == o["cap"]).all()
    vc = pv.PlonkVanishingCircuit(o["c"].log_n, o["params"], o["circ"], cases.CAP_HEIGHT, len(o["pis"]))
    ofp, ffp = (fri(log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4) for log_n in (vc.log_n, FRI_LOG_N))
    c1, c2 = _ctx(vc.log_n, (80, 8, 2), to_params(ofp), vc.circuit()), _ctx(FRI_LOG_N, (80, 8, 2), to_params(ffp), vc.circuit())
    ver = pv.PlonkProofVerifier(c1, o["c"].log_n, o["params"], o["circ"], to_params(o["ofp"]), len(o["pis"]), fri_ctx=c2,
                                fri=(to_params(ofp), to_params(ffp)), digest=DIGEST)
    assert ver.fc.log_n == FRI_LOG_N and ver.vc.log_n == vc.log_n
    yield {"o": o, "inner": inner, "proof": proof, "ver": ver, "c": ver.vc, "ofp": ofp, "cs": ver.vc.constants_sigmas(),
           "args": pv.flat_proof_arguments(ver.vc, proof, cases.INNER_DIGEST)}
    ver.close()
    inner.close()
    for c in (c1, c2, ic):
        c.close()


@pytest.fixture(scope="module", params=cases.NAMES)
def whole(request):
    yield from _case(request.param)


@pytest.fixture(scope="module")
def ragged():
    yield from _case("ragged")


def _reference(b):
    """the reading's table of the case, once: (public inputs, their hash, the partial witness, the replayed witness)"""
    if "reference" not in b:
        c = b["c"]
        pis = c.public_inputs(*b["args"])
        pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
        pw = c.partial_witness(*b["args"])
        b["reference"] = (pis, pih, pw, rd.replay(pw, b["cs"][:c.num_constants], c.generators(), pih, c.schedule()))
    return b["reference"]


def test_the_device_makes_the_oracles_inner_proof(whole):
    want = cases.oracle_proof(whole["o"])
    assert len(whole["proof"]) == len(want) and (whole["proof"] == want).all()


def test_the_device_witness_is_the_reading_on_every_route(ctx, whole):
    import sipp_amd
    b, circ, L = whole, whole["c"], sipp_amd.lib()
    pis, pih, pw, want = _reference(b)
    r = read(b["o"], b["proof"])
    at = lambda cell: int(want[cell[0], cell[1]])
    assert tuple(at(x) for x in circ.zeta_cells) == r["zeta"] and [tuple(at(x) for x in t) for t in circ.term_cells] == r["terms"]
    assert [tuple(tuple(at(x) for x in s) for s in sd) for sd in circ.side_cells] == r["sides"]
    sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
    d_c = dev(b["cs"][:circ.num_constants])
    try:
        for route in (0, NO_GRAPH, INTERP_ONE_LANE, REDUCE_ONE_LANE):
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            d_w = dev(pw)
            ctx.plonk_generate_witness_levels(d_w, d_c, circ.log_n, circ.generators(), pih, sched)
            assert first_mismatch(host(d_w), want) is None, route
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_the_outer_proof_is_the_oracles_and_proves_from_the_inner_proofs_words(whole):
    b, circ = whole, whole["c"]
    pr = b["ver"].vanishing
    pis, pih, pw, want = _reference(b)
    assert (pr.cap == _oracle.Batch(b["cs"], circ.log_n, rate_bits=3, cap_height=4).cap).all()
    pf = pr.prove(*b["args"])
    ref = _oracle.plonk_prove_gates(want, b["cs"], circ.log_n, OUTER, b["ofp"], pr.circuit, DIGEST, pis)
    assert len(pf) == len(ref) and (pf == ref).all()
    assert pr.verify(pf) == (0, 0) and _oracle.plonk_verify_gates(pf, pr.cap, OUTER, b["ofp"], pr.circuit, DIGEST) == 0
    for _ in range(2):
        words = pr.prove_proof(b["proof"], cases.INNER_DIGEST)
        assert len(words) == len(pf) and (words == pf).all()


@pytest.mark.parametrize("what", TAMPERS)
def test_tampered_inner_proofs_are_refused_and_the_prover_goes_on(ragged, what):
    b = ragged
    pr = b["ver"].vanishing
    pf, digest = tampered(b, what)
    bad = pr.prove_proof(pf, digest)
    assert pr.verify(bad)[0] != 0 and _oracle.plonk_verify_gates(bad, pr.cap, OUTER, b["ofp"], pr.circuit, DIGEST) != 0
    assert pr.verify(pr.prove_proof(b["proof"], cases.INNER_DIGEST)) == (0, 0)


def test_the_pair_is_accepted_and_a_stitched_pair_is_refused(whole):
    b, o, ver = whole, whole["o"], whole["ver"]
    pair = ver.prove_proof(b["proof"], o["cap"], cases.INNER_DIGEST)
    assert ver.verify(pair, o["cap"], cases.INNER_DIGEST) == o["pis"]
    # another inner proof of the same circuit: other public inputs (basic, ragged) or another leaf (poseidon)
    c = o["c"]
    if o["name"] == "poseidon":
        from oracle.py import plonky2_generic as g2
        leaves = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 17]]
        tree = g2.MerkleTree(leaves, 1)
        args = ([v for d in tree.cap for v in d], [3], [leaves[3]], [tree.prove(3)])
        pis, pw = c.public_inputs(*args[:3]), c.partial_witness(*args)
    else:
        args = ([6, 1, 2, 3, 4], 1)
        pis, pw = c.public_inputs(args[0]), c.partial_witness(*args)
    other = b["inner"].data.prove(pw, pis)
    assert b["inner"].verify(other) == (0, 0)
    pair2 = ver.prove_proof(other, o["cap"], cases.INNER_DIGEST)
    assert ver.verify(pair2, o["cap"], cases.INNER_DIGEST) == [int(v) for v in pis]
    for stitched in ((pair[0], pair2[1]), (pair2[0], pair[1])):
        with pytest.raises(ValueError, match="differ"):
            ver.verify(stitched, o["cap"], cases.INNER_DIGEST)
