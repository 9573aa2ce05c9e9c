"""The whole FRI query round in the outer circuit on the device (sipp_amd/fri_verifier.py): opening proofs made by the device, read by
tests/_fri_round_reading.py into FriVerifierProver; the device witness under every launch route against the Python reading
(tests/_witness_reading.py) cell for cell; the proof word for word the oracle's of the read witness, accepted by both verifiers, refused
when any part of the opening proof is tampered with; sipp_circuit_prove_inputs against the dense call and at its refusals."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import fri_verifier as fv
from sipp_amd import merkle as mk
from tests import _fri_cases as fc
from tests import _fri_round_reading as rr
from tests import _oracle
from tests import _witness_reading as rd
from tests._device import INTERP_ONE_LANE, NO_GRAPH, REDUCE_ONE_LANE, dev, first_mismatch, host
from tests.test_fri_verifier_circuit import CASES, ROUND_A16, SHAPES, TAMPERS, tampered
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

DIGEST = (85, 86, 87, 88)


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)
    yield c
    c.close()


def _other_transcript(case):
    """the same oracles behind another transcript prefix: other challenges, other queries"""
    return fc.Case(case.id + "-second", log_n=case.log_n, rate_bits=case.rate_bits, cap_height=case.cap_height, widths=case.widths,
                   seed=case.seed, fri=case.fri, prefix=(9, 8, 7))


def _read(ctx, case0):
    """two opening proofs made by the DEVICE (sipp_fri_prove_openings, equal to the oracle's word for word) and their data"""
    from tests.test_gpu_fri_edges import commit, prove_and_compare
    out = []
    for case in (case0, _other_transcript(case0)):
        inst = fc.build(case)
        devs, keep = commit(ctx, inst)
        pf, _ = prove_and_compare(ctx, inst, devs, fc.challenger(case))
        args, shape, _ = rr.round_data(inst, pf)
        assert shape == SHAPES[case0.id]
        out.append(args)
        del devs, keep
    assert out[0][7] != out[1][7]                               # other queries
    return out


def _prover(shape):
    import sipp_amd
    circ = fv.FriQueryRoundCircuit(*shape)
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc))
    c = sipp_amd.Ctx(workspace_bytes=ws)
    return fv.FriVerifierProver(c, *shape, fri=gfp, digest=DIGEST), c, ofp


def _reference(circ, cs, args):
    """the reading's table of the arguments, once: (public inputs, their hash, the partial witness, the replayed witness)"""
    pis = circ.public_inputs(*args[:8])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    pw = circ.partial_witness(*args)
    return pis, pih, pw, rd.replay(pw, cs[:circ.num_constants], circ.generators(), pih, circ.schedule())


@pytest.fixture(scope="module", params=CASES, ids=repr)
def joined(ctx, request):
    """per shape: the prover, and per transcript the arguments with the reading's table"""
    data = _read(ctx, request.param)
    pr, c, ofp = _prover(SHAPES[request.param.id])
    cs = pr.circ.constants_sigmas()
    yield pr, ofp, cs, [(args,) + _reference(pr.circ, cs, args) for args in data]
    pr.close()
    c.close()


@pytest.fixture(scope="module")
def joined16(ctx):
    data = _read(ctx, ROUND_A16)
    pr, c, ofp = _prover(SHAPES["round-a16"])
    yield pr, ofp, data[0]
    pr.close()
    c.close()


def _verdicts(pr, ofp, pf):
    return pr.verify(pf), _oracle.plonk_verify_gates(pf, pr.cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST)


def test_the_device_witness_is_the_reading_on_every_route(ctx, joined):
    import sipp_amd
    pr, ofp, cs, refs = joined
    circ, L = pr.circ, sipp_amd.lib()
    sched = sipp_amd.PlonkSchedule.from_dict(circ.schedule())
    d_c = dev(cs[:circ.num_constants])
    try:
        for args, pis, pih, pw, want in refs:
            for route in (0, INTERP_ONE_LANE, REDUCE_ONE_LANE, NO_GRAPH):
                assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
                d_w = dev(pw)
                ctx.plonk_generate_witness_levels(d_w, d_c, circ.log_n, circ.generators(), pih, sched)
                assert first_mismatch(host(d_w), want) is None, route
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_the_query_rounds_of_a_device_opening_proof_prove_and_verify(joined):
    pr, ofp, cs, refs = joined
    circ = pr.circ
    assert (pr.cap == _oracle.Batch(cs, circ.log_n, rate_bits=3, cap_height=4).cap).all()
    for round_, (args, pis, pih, pw, want) in enumerate(refs):     # the second opening proof goes through the same circuit data
        pf = pr.prove(*args)
        ref = _oracle.plonk_prove_gates(want, cs, circ.log_n, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST, pis)
        assert len(pf) == len(ref) and (pf == ref).all(), round_
        assert _verdicts(pr, ofp, pf) == ((0, 0), 0)
        dense = pr.data.prove(pw, pis)                              # sipp_circuit_prove_inputs against the dense call
        assert len(dense) == len(pf) and (dense == pf).all(), round_


@pytest.mark.parametrize("what", TAMPERS)
def test_tampered_inputs_are_refused_and_the_prover_goes_on(joined16, what):
    pr, ofp, args = joined16
    pf = pr.prove(*tampered(args, what))
    (st, stage), orc = _verdicts(pr, ofp, pf)
    assert st != 0 and orc != 0, (st, stage, orc)
    good = pr.prove(*args)
    assert _verdicts(pr, ofp, good) == ((0, 0), 0)


# ---- sipp_circuit_prove_inputs --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def merkle():
    """MerkleOpeningCircuit(3, 1, 1, 1) with the opening of a two-leaf tree by the oracle's hash"""
    import sipp_amd
    from oracle.py import plonky2_generic as g2
    circ = mk.MerkleOpeningCircuit(3, 1, 1, 1)
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    c = sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc)))
    pr = mk.MerkleOpeningProver(c, 3, 1, 1, 1, fri=gfp, digest=DIGEST)
    leaves = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 16]]
    tree = g2.MerkleTree(leaves, 1)
    args = ([v for d in tree.cap for v in d], [3], [leaves[3]], [tree.prove(3)])
    yield pr, ofp, args
    pr.close()
    c.close()


def _pairs(circ, args):
    """the input cells of a partial witness: the cycles of the public inputs and, of the Merkle circuit, the sibling cells"""
    pw = circ.partial_witness(*args)
    cells = [x for cyc in circ.pi_cycle for x in cyc] + [x for path in getattr(circ, "sibling_cells", []) for lvl in path for x in lvl]
    cells = np.array(sorted(set(cells)), dtype=np.uint64)
    vals = pw.reshape(-1)[cells.astype(np.int64)]
    w = np.zeros_like(pw)
    w.reshape(-1)[cells.astype(np.int64)] = vals
    assert (w == pw).all()
    return pw, cells, vals


def test_prove_inputs_is_the_dense_proof_on_the_merkle_circuit(merkle):
    pr, ofp, args = merkle
    circ = pr.circ
    pis = circ.public_inputs(*args[:3])
    pw, cells, vals = _pairs(circ, args)
    dense = pr.data.prove(pw, pis)
    assert _verdicts(pr, ofp, dense) == ((0, 0), 0)
    got = pr.data.prove_inputs(cells, vals, pis)
    assert len(got) == len(dense) and (got == dense).all()
    # the order of the pairs does not matter; a pair given twice with one value is accepted
    again = pr.data.prove_inputs(np.concatenate([cells[::-1], cells[:5]]), np.concatenate([vals[::-1], vals[:5]]), pis)
    assert len(again) == len(dense) and (again == dense).all()


def test_prove_inputs_stores_any_word_as_the_dense_call_does(merkle):
    """values are stored as given: a non-canonical word in an input cell gives the dense call's proof of the same table"""
    pr, ofp, args = merkle
    circ = pr.circ
    pis = circ.public_inputs(*args[:3])
    pw, cells, vals = _pairs(circ, args)
    vals = vals.copy()
    vals[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    pw = pw.copy()
    pw.reshape(-1)[int(cells[-1])] = vals[-1]
    dense, got = pr.data.prove(pw, pis), pr.data.prove_inputs(cells, vals, pis)
    assert len(got) == len(dense) and (got == dense).all()


@pytest.mark.parametrize("which", ["merkle", "joined"])
def test_prove_inputs_refuses_conflicts_and_cells_outside_the_table_and_goes_on(merkle, joined16, which):
    import sipp_amd
    if which == "merkle":
        pr, ofp, args = merkle
        pis = pr.circ.public_inputs(*args[:3])
        _, cells, vals = _pairs(pr.circ, args)
    else:
        pr, ofp, args = joined16
        pis = pr.circ.public_inputs(*args[:8])
        cells, vals = pr.circ.input_cells(*args)
    good = pr.data.prove_inputs(cells, vals, pis)
    assert _verdicts(pr, ofp, good) == ((0, 0), 0)
    k = len(cells) // 2
    conflict = (np.append(cells, cells[k]), np.append(vals, vals[k] ^ np.uint64(1)))
    outside = (np.append(cells, np.uint64(pr.circ.num_wires * pr.circ.n)), np.append(vals, np.uint64(1)))
    far = (np.append(cells, np.uint64(1 << 63)), np.append(vals, np.uint64(1)))
    for bad in (conflict, outside, far, conflict):
        with pytest.raises(sipp_amd.SippError) as e:
            pr.data.prove_inputs(bad[0], bad[1], pis)
        assert e.value.code == -1                                   # SIPP_E_BADARG
        again = pr.data.prove_inputs(cells, vals, pis)
        assert len(again) == len(good) and (again == good).all()


def test_prove_inputs_without_pairs_is_served_and_the_verifier_judges(merkle):
    """n_inputs = 0 with NULL arrays: the call proves the zero table; this circuit's public inputs are then not its cells', which the
    verifiers refuse"""
    pr, ofp, args = merkle
    pis = pr.circ.public_inputs(*args[:3])
    empty = np.zeros(0, dtype=np.uint64)
    pf = pr.data.prove_inputs(empty, empty, pis)
    dense = pr.data.prove(np.zeros((pr.circ.num_wires, pr.circ.n), dtype=np.uint64), pis)
    assert len(pf) == len(dense) and (pf == dense).all()
    (st, _), orc = _verdicts(pr, ofp, pf)
    assert st != 0 and orc != 0
