"""The vanishing circuit with the inner Poseidon gate through MDS rows and the closing Horner in chunks of 8, on the device
(sipp_amd/plonk_vanishing.py, poseidon_mds and alpha_chunk; SIPP_GEN_POSEIDON_MDS in witness.hip): the `poseidon` case of
tests/_plonk_vanishing_cases.py, its inner proof made by the device; the device witness under the graph and the launch-by-launch route
against the Python readings cell for cell; prove_proof from the inner proof's words word for word the oracle's outer proof of the read
witness, accepted by both verifiers; the pair of PlonkProofVerifier accepted with the inner public inputs, a pair stitched from two
inner proofs refused.  The inner circuit's and the vanishing circuit's tables are 2^10 rows."""
import numpy as np
import pytest

from sipp_amd import plonk_vanishing as pv
from tests import _challenger_reading  # noqa: F401  (registers the reading of generator kind 15)
from tests import _oracle
from tests import _plonk_vanishing_cases as cases
from tests import _poseidon_mds_reading as pm
from tests import _witness_reading as rd
from tests._device import NO_GRAPH, dev, first_mismatch, host
from tests.test_gpu_fri_generic import to_params
from tests.test_gpu_plonk_vanishing_circuit import DIGEST, FRI_LOG_N, OUTER, _ctx, _inner_prover
from tests.test_oracle_plonk import fri
from tests.test_plonk_vanishing_circuit import read

pytestmark = pytest.mark.gpu

KW = dict(poseidon_mds=True, alpha_chunk=8)


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def whole():
    """the inner proof by the DEVICE, the verifier pair built for it under both keywords, the arguments, the reading's table"""
    o = cases.inner("poseidon")
    inner, ic = _inner_prover(o)
    proof = inner.data.prove(o["pw"], o["pis"])
    assert inner.verify(proof) == (0, 0) and (inner.cap == o["cap"]).all()
    vc = pv.PlonkVanishingCircuit(o["c"].log_n, o["params"], o["circ"], cases.CAP_HEIGHT, len(o["pis"]), **KW)
    assert vc.log_n == 10 and len(vc.mds_rows) == 30 and pm.GEN_POSEIDON_MDS in [g[0] for g in vc.generators()]
    ofp, ffp = (fri(log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4) for log_n in (vc.log_n, FRI_LOG_N))
    c1, c2 = _ctx(vc.log_n, (80, 8, 2), to_params(ofp), vc.circuit()), _ctx(FRI_LOG_N, (80, 8, 2), to_params(ffp), vc.circuit())
    ver = pv.PlonkProofVerifier(c1, o["c"].log_n, o["params"], o["circ"], to_params(o["ofp"]), len(o["pis"]), fri_ctx=c2,
                                fri=(to_params(ofp), to_params(ffp)), digest=DIGEST, **KW)
    c = ver.vc
    assert ver.fc.log_n == FRI_LOG_N and c.log_n == 10 and c.generators() == vc.generators()
    cs = c.constants_sigmas()
    args = pv.flat_proof_arguments(c, proof, cases.INNER_DIGEST)
    pis = c.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    pw = c.partial_witness(*args)
    want = rd.replay(pw, cs[:c.num_constants], c.generators(), pih, c.schedule())
    yield {"o": o, "inner": inner, "proof": proof, "ver": ver, "c": c, "ofp": ofp, "cs": cs, "args": args, "pis": pis, "pih": pih, "pw": pw,
           "want": want}
    ver.close()
    inner.close()
    for x in (c1, c2, ic):
        x.close()


def test_the_device_witness_is_the_reading_under_the_graph_and_launch_by_launch(ctx, whole):
    import sipp_amd
    b, circ, L = whole, whole["c"], sipp_amd.lib()
    want = b["want"]
    r = read(b["o"], b["proof"])
    at = lambda cell: int(want[cell[0], cell[1]])
    assert tuple(at(x) for x in circ.zeta_cells) == r["zeta"] and [tuple(at(x) for x in t) for t in circ.term_cells] == r["terms"]
    assert [tuple(tuple(at(x) for x in s) for s in sd) for sd in circ.side_cells] == r["sides"]
    assert want.shape == (135, 1 << 10)
    sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
    d_c = dev(b["cs"][:circ.num_constants])
    try:
        for route in (0, 0, NO_GRAPH):                          # the captured graph, its replay, the launches one by one
            assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
            d_w = dev(b["pw"])
            ctx.plonk_generate_witness_levels(d_w, d_c, circ.log_n, circ.generators(), b["pih"], sched)
            assert first_mismatch(host(d_w), want) is None, route
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_the_outer_proof_from_the_inner_proofs_words_is_the_oracles(whole):
    b, circ = whole, whole["c"]
    pr = b["ver"].vanishing
    assert (pr.cap == _oracle.Batch(b["cs"], circ.log_n, rate_bits=3, cap_height=4).cap).all()
    ref = _oracle.plonk_prove_gates(b["want"], b["cs"], circ.log_n, OUTER, b["ofp"], pr.circuit, DIGEST, b["pis"])
    for _ in range(2):
        words = pr.prove_proof(b["proof"], cases.INNER_DIGEST)
        assert len(words) == len(ref) and (words == ref).all()
    assert pr.verify(ref) == (0, 0) and _oracle.plonk_verify_gates(ref, pr.cap, OUTER, b["ofp"], pr.circuit, DIGEST) == 0


def test_the_pair_is_accepted_and_a_stitched_pair_is_refused(whole):
    from oracle.py import plonky2_generic as g2
    b, o, ver = whole, whole["o"], whole["ver"]
    pair = ver.prove_proof(b["proof"], o["cap"], cases.INNER_DIGEST)
    assert ver.verify(pair, o["cap"], cases.INNER_DIGEST) == o["pis"]
    c = o["c"]
    leaves = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 17]]                        # another leaf under another cap
    tree = g2.MerkleTree(leaves, 1)
    args = ([v for d in tree.cap for v in d], [3], [leaves[3]], [tree.prove(3)])
    pis, pw = c.public_inputs(*args[:3]), c.partial_witness(*args)
    other = b["inner"].data.prove(pw, pis)
    assert b["inner"].verify(other) == (0, 0)
    pair2 = ver.prove_proof(other, o["cap"], cases.INNER_DIGEST)
    assert ver.verify(pair2, o["cap"], cases.INNER_DIGEST) == [int(v) for v in pis]
    for stitched in ((pair[0], pair2[1]), (pair2[0], pair[1])):
        with pytest.raises(ValueError, match="differ"):
            ver.verify(stitched, o["cap"], cases.INNER_DIGEST)
