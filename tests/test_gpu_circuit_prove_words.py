"""sipp_circuit_set_input_map / sipp_circuit_prove_words on the device: on the smallest pinned FriProofCircuit shape (round-a16, an opening
proof by the oracle) and on `basic` (tests/_basic_circuit.py) the proof from the words is sipp_circuit_prove_inputs' word for word; the
map at its edges (empty, a cell twice, a bad cell or source, replaced, missing, another length); build / destroy gives the map's memory
back."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import circuit as ci
from sipp_amd import fri_proof as fp
from tests import _oracle
from tests._basic_circuit import BasicCircuit
from tests.test_fri_proof_circuit import build, circuit_kw
from tests.test_fri_verifier_circuit import ROUND_A16, SHAPES
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

DIGEST = (89, 90, 91, 92)
BADARG = -1
PIS, INDEX = [13, 3, _oracle.P - 1, 5, 1 << 40], 2


def _ctx_for(circ, gfp):
    import sipp_amd
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(circ.circuit())
    return sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc)))


@pytest.fixture(scope="module")
def whole16():
    """the opening proof of round-a16 by the oracle, and the prover with its map set at build"""
    o = build(ROUND_A16)
    ofp = fri(o["c"].log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    c = _ctx_for(o["c"], to_params(ofp))
    pr = fp.FriProofProver(c, *SHAPES[ROUND_A16.id], fri=to_params(ofp), digest=DIGEST, **circuit_kw(ROUND_A16))
    yield pr, ofp, o
    pr.close()
    c.close()


@pytest.fixture(scope="module")
def basic():
    """-> (the prover, the oracle's FRI parameters, cells, values, public inputs, the proof of sipp_circuit_prove_inputs)"""
    circ = BasicCircuit()
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    c = _ctx_for(circ, to_params(ofp))
    pr = ci.CircuitProver(c, circ, fri=to_params(ofp), digest=DIGEST)
    cells, vals = circ.input_cells(PIS, INDEX)
    pis = circ.public_inputs(PIS)
    yield pr, ofp, cells, vals, pis, pr.data.prove_inputs(cells, vals, pis)
    pr.close()
    c.close()


def _scrambled(vals, n_words, n_extra, seed):
    """values at random places of words || extra, the other words noise -> (words, extra, sources)"""
    rng = np.random.default_rng(seed)
    staged = rng.integers(0, 1 << 63, size=n_words + n_extra, dtype=np.uint64)
    sources = rng.permutation(n_words + n_extra)[:len(vals)].astype(np.uint64)
    staged[sources.astype(np.int64)] = vals
    return staged[:n_words], staged[n_words:], sources


def test_fri_proof_circuit_proves_from_the_proofs_words(whole16):
    pr, ofp, o = whole16
    c, data = pr.circ, o["data"]
    assert pr.data.input_map == (c.proof_words, len(c.pi_other))
    want = pr.data.prove_inputs(*c.proof_inputs(o["proof"], data["caps"], data["points"], o["transcript"]))
    assert pr.verify(want) == (0, 0)
    assert _oracle.plonk_verify_gates(want, pr.cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST) == 0
    for _ in range(2):                                          # the second proof finds the table as the first left it
        got = pr.prove_proof(o["proof"], data["caps"], data["points"], o["transcript"])
        assert len(got) == len(want) and (got == want).all()
    words, extra, pis = c.words_of_proof(o["proof"], data["caps"], data["points"], o["transcript"])
    got = pr.data.prove_words(words, extra, pis)
    assert len(got) == len(want) and (got == want).all()
    # an opening proof with its last sibling word changed goes through the same map: served, refused by the verifier, a good proof next
    bad = o["proof"].copy()
    bad[-1] ^= np.uint64(1)
    assert pr.verify(pr.data.prove_words(*c.words_of_proof(bad, data["caps"], data["points"], o["transcript"])))[0] != 0
    assert (pr.data.prove_words(words, extra, pis) == want).all()


def test_basic_proves_from_words_and_both_verifiers_accept(basic):
    pr, ofp, cells, vals, pis, want = basic
    assert pr.verify(want) == (0, 0)
    assert _oracle.plonk_verify_gates(want, pr.cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST) == 0
    for n_words, n_extra, seed in ((len(vals), 0, 1), (0, len(vals) + 3, 2), (1000, 77, 3)):
        words, extra, sources = _scrambled(vals, n_words, n_extra, seed)
        pr.data.set_input_map(cells, sources, n_words, n_extra)              # each call replaces the map before
        got = pr.data.prove_words(words, extra, pis)
        assert len(got) == len(want) and (got == want).all(), (n_words, n_extra)


def test_the_map_at_its_edges(basic):
    import sipp_amd
    pr, ofp, cells, vals, pis, want = basic
    d, total = pr.data, pr.circ.num_wires * pr.circ.n
    # a cell mapped twice: to one word, to two equal words, to two different words
    words, extra, sources = _scrambled(vals, 300, 20, 4)
    twice = np.concatenate([cells, cells[:3]])
    d.set_input_map(twice, np.concatenate([sources, sources[:3]]), 300, 20)
    assert (d.prove_words(words, extra, pis) == want).all()
    spare = np.setdiff1d(np.arange(320, dtype=np.uint64), sources)[:3]
    staged = np.concatenate([words, extra])
    staged[spare.astype(np.int64)] = vals[:3]
    d.set_input_map(twice, np.concatenate([sources, spare]), 300, 20)
    assert (d.prove_words(staged[:300], staged[300:], pis) == want).all()
    staged[int(spare[1])] ^= np.uint64(1)
    with pytest.raises(sipp_amd.SippError) as e:
        d.prove_words(staged[:300], staged[300:], pis)
    assert e.value.code == BADARG
    staged[int(spare[1])] ^= np.uint64(1)
    assert (d.prove_words(staged[:300], staged[300:], pis) == want).all()    # a good proof follows
    # a bad cell or source leaves the map before in force
    for bad_cells, bad_sources in ((np.append(cells, np.uint64(total)), np.append(sources, np.uint64(0))),
                                   (np.append(cells, np.uint64(0)), np.append(sources, np.uint64(320))),
                                   (cells, np.where(np.arange(len(sources)) == len(sources) - 1, np.uint64(1 << 63), sources))):
        with pytest.raises(sipp_amd.SippError) as e:
            d.set_input_map(bad_cells, bad_sources, 300, 20)
        assert e.value.code == BADARG
        assert d.input_map == (300, 20) and (d.prove_words(staged[:300], staged[300:], pis) == want).all()
    # the last cell of the table and the last staged word are in range
    d.set_input_map(np.append(cells, np.uint64(total - 1)), np.append(sources, np.uint64(319)), 300, 20)
    assert d.verify(d.prove_words(staged[:300], staged[300:], pis)) == (0, 0)               # an unrouted cell of a Noop row binds nothing
    d.set_input_map(twice, np.concatenate([sources, spare]), 300, 20)
    # other lengths than the map's
    for w, x in ((staged[:299], staged[300:]), (staged[:300], staged[300:319]), (staged[:301], staged[301:]), (staged[:0], staged[:0])):
        with pytest.raises(sipp_amd.SippError) as e:
            d.prove_words(w, x, pis)
        assert e.value.code == BADARG
    assert (d.prove_words(staged[:300], staged[300:], pis) == want).all()
    # the empty map: the proof of sipp_circuit_prove_inputs without pairs
    none = np.zeros(0, dtype=np.uint64)
    d.set_input_map(none, none, 0, 0)
    empty = d.prove_words(none, none, pis)
    assert (empty == d.prove_inputs(none, none, pis)).all() and not (empty[:64] == want[:64]).all()
    d.set_input_map(none, none, 5, 2)                           # words nobody reads
    assert (d.prove_words(staged[:5], staged[:2], pis) == empty).all()
    # and after all that the pairs still prove as before
    assert (d.prove_inputs(cells, vals, pis) == want).all()


def test_no_map_no_proof_and_destroy_returns_the_maps_memory(basic):
    import sipp_amd
    from sipp_amd._lib import device_free_bytes
    pr, ofp, cells, vals, pis, want = basic
    circ, ctx = pr.circ, pr.data.ctx
    build_ = lambda: sipp_amd.CircuitData(ctx, circ.log_n, pr.params, pr.fri, pr._pc, circ.constants_sigmas(), circ.generators(),
                                          sched=circ.schedule(), digest=DIGEST)
    d = build_()
    try:
        with pytest.raises(sipp_amd.SippError) as e:
            d.prove_words(vals, vals[:0], pis)
        assert e.value.code == BADARG and d.input_map is None
        d.set_input_map(cells, np.arange(len(cells)), len(cells), 0)
        assert (d.prove_words(vals, vals[:0], pis) == want).all()
    finally:
        d.close()
    # a map of 4M pairs is 64 MB: a replaced map goes at once, the last one with the data
    big = 1 << 22
    big_cells, big_sources = np.resize(cells, big), np.resize(np.arange(len(cells), dtype=np.uint64), big)
    free0 = device_free_bytes(0)
    for _ in range(3):
        d = build_()
        free1 = device_free_bytes(0)
        d.set_input_map(big_cells, big_sources, len(cells), 0)
        d.set_input_map(big_cells, big_sources, len(cells), 0)
        assert (48 << 20) < free1 - device_free_bytes(0) < (96 << 20)
        assert (d.prove_words(vals, vals[:0], pis) == want).all()
        d.close()
    assert abs(device_free_bytes(0) - free0) < (8 << 20)
