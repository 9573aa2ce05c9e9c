"""The whole of verify_fri_proof in the outer circuit on the device (sipp_amd/fri_proof.py): opening proofs made by the device, two
transcripts per shape through one circuit data; the device witness under every launch route against the Python reading
(tests/_witness_reading.py with tests/_challenger_reading.py's kind 15) cell for cell; the proof word for word the oracle's of the read
witness, accepted by both verifiers; prove_proof (the inputs gathered from the flat proof's words) against prove(*arguments); tampered
proofs refused, the prover going on."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import fri_proof as fp
from tests import _challenger_reading as cr
from tests import _fri_cases as fc
from tests import _fri_round_reading as rr
from tests import _oracle
from tests import _witness_reading as rd
from tests._device import INTERP_ONE_LANE, NO_GRAPH, REDUCE_ONE_LANE, dev, first_mismatch, host
from tests.test_fri_proof_circuit import TAMPERS, arguments, circuit_kw, reading, tampered
from tests.test_fri_verifier_circuit import CASES, ROUND_A16, SHAPES
from tests.test_gpu_fri_generic import to_params
from tests.test_gpu_fri_verifier_circuit import _other_transcript
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

DIGEST = (89, 90, 91, 92)


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)
    yield c
    c.close()


def _read(ctx, case0):
    """two opening proofs made by the DEVICE (sipp_fri_prove_openings, equal to the oracle's word for word) behind two transcripts that
    leave as many inputs pending: per proof what a caller has (the flat proof, the caps, the points, the arriving transcript)"""
    from tests.test_gpu_fri_edges import commit, prove_and_compare
    out = []
    for case in (case0, _other_transcript(case0)):
        inst = fc.build(case)
        devs, keep = commit(ctx, inst)
        pf, _ = prove_and_compare(ctx, inst, devs, fc.challenger(case))
        _, shape, data = rr.round_data(inst, pf)
        assert shape == SHAPES[case0.id] and circuit_kw(case) == circuit_kw(case0)
        transcript = cr.arriving(case)[0]
        out.append({"case": case0, "proof": np.asarray(pf, dtype=np.uint64), "data": data, "transcript": transcript,
                    "drawn": reading(case, shape, pf, transcript)})
        del devs, keep
    assert out[0]["drawn"]["x_index"] != out[1]["drawn"]["x_index"] and out[0]["drawn"]["alpha"] != out[1]["drawn"]["alpha"]
    return out


def _prover(case):
    import sipp_amd
    shape, kw = SHAPES[case.id], circuit_kw(case)
    circ = fp.FriProofCircuit(*shape, **kw)
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc))
    c = sipp_amd.Ctx(workspace_bytes=ws)
    return fp.FriProofProver(c, *shape, fri=gfp, digest=DIGEST, **kw), c, ofp


def _reference(circ, cs, o):
    """the reading's table of one opening proof, once: (arguments, public inputs, their hash, the partial witness, the replayed witness)"""
    args = arguments(circ, o["proof"], o["data"], o["transcript"])
    pis = circ.public_inputs(*args[:6])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    pw = circ.partial_witness(*args)
    return args, pis, pih, pw, rd.replay(pw, cs[:circ.num_constants], circ.generators(), pih, circ.schedule())


@pytest.fixture(scope="module", params=CASES, ids=repr)
def whole(ctx, request):
    """per shape: the prover, and per transcript the opening proof with the reading's table"""
    data = _read(ctx, request.param)
    pr, c, ofp = _prover(request.param)
    cs = pr.circ.constants_sigmas()
    yield pr, ofp, cs, [(o,) + _reference(pr.circ, cs, o) for o in data]
    pr.close()
    c.close()


@pytest.fixture(scope="module")
def whole16(ctx):
    data = _read(ctx, ROUND_A16)
    pr, c, ofp = _prover(ROUND_A16)
    o = data[0]
    o["args"] = arguments(pr.circ, o["proof"], o["data"], o["transcript"])
    yield pr, ofp, o
    pr.close()
    c.close()


def _verdicts(pr, ofp, pf):
    return pr.verify(pf), _oracle.plonk_verify_gates(pf, pr.cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST)


def test_the_device_witness_is_the_reading_on_every_route(ctx, whole):
    import sipp_amd
    pr, ofp, cs, refs = whole
    circ, L = pr.circ, sipp_amd.lib()
    sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
    d_c = dev(cs[:circ.num_constants])
    try:
        for o, args, pis, pih, pw, want in refs:
            d = o["drawn"]                                      # the reading's table holds what the oracle's Challenger draws
            assert tuple(int(want[x[0], x[1]]) for x in circ.alpha_cells) == d["alpha"]
            assert [int(want[x[0], x[1]]) for x in circ.index_cells] == d["challenges"]
            assert [int(want[0, r]) for r in circ.cap_sum_row] == d["cap_index"]
            for route in (0, INTERP_ONE_LANE, REDUCE_ONE_LANE, NO_GRAPH):
                assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
                d_w = dev(pw)
                ctx.plonk_generate_witness_levels(d_w, d_c, circ.log_n, circ.generators(), pih, sched)
                assert first_mismatch(host(d_w), want) is None, route
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_a_device_opening_proof_proves_and_verifies_from_its_words(whole):
    pr, ofp, cs, refs = whole
    circ = pr.circ
    assert (pr.cap == _oracle.Batch(cs, circ.log_n, rate_bits=3, cap_height=4).cap).all()
    for round_, (o, args, pis, pih, pw, want) in enumerate(refs):  # the second opening proof goes through the same circuit data
        pf = pr.prove(*args)
        ref = _oracle.plonk_prove_gates(want, cs, circ.log_n, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST, pis)
        assert len(pf) == len(ref) and (pf == ref).all(), round_
        assert _verdicts(pr, ofp, pf) == ((0, 0), 0)
        words = pr.prove_proof(o["proof"], o["data"]["caps"], o["data"]["points"], o["transcript"])
        assert len(words) == len(pf) and (words == pf).all(), round_


@pytest.mark.parametrize("what", TAMPERS)
def test_tampered_proofs_are_refused_and_the_prover_goes_on(whole16, what):
    pr, ofp, o = whole16
    pf = pr.prove(*tampered(o, what))
    (st, stage), orc = _verdicts(pr, ofp, pf)
    assert st != 0 and orc != 0, (st, stage, orc)
    good = pr.prove_proof(o["proof"], o["data"]["caps"], o["data"]["points"], o["transcript"])
    assert _verdicts(pr, ofp, good) == ((0, 0), 0)
