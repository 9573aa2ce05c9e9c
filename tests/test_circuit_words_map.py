"""The maps behind sipp_circuit_set_input_map on the CPU: FriProofCircuit.words_map / words_of_proof against proof_inputs, and the
`basic` circuit of tests/_basic_circuit.py (replayed, satisfied, proved and judged by the oracle and the library's verifier); the new
entry points in the library and in every binding."""
import os

import numpy as np
import pytest

from tests import _oracle
from tests import _witness_reading as rd
from tests._basic_circuit import BasicCircuit
from tests.test_fri_proof_circuit import build
from tests.test_fri_verifier_circuit import ROUND_A16, prove_and_judge, satisfied

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIS, INDEX = [13, 3, _oracle.P - 1, 5, 1 << 40], 2


def test_the_library_and_the_bindings_have_the_two_calls():
    import sipp_amd
    from sipp_amd import _lib
    L = sipp_amd.lib()
    for name in ("sipp_circuit_set_input_map", "sipp_circuit_prove_words"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
        assert name in open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
        assert "ffi::" + name in open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read()
        assert name in open(os.path.join(ROOT, "include", "sipp_host.hpp")).read()
    # a null circuit data is refused before anything is read
    assert L.sipp_circuit_set_input_map(None, None, None, 0, 0, 0) == -1
    assert L.sipp_circuit_prove_words(None, None, 0, None, 0, None, 0, None, 0, None) == -1


def test_words_map_and_words_of_proof_are_proof_inputs():
    o = build(ROUND_A16)
    c, data = o["c"], o["data"]
    cells, sources, n_words, n_extra = c.words_map()
    assert cells.dtype == sources.dtype == np.uint64 and cells.shape == sources.shape
    assert n_words == c.proof_words == len(o["proof"]) and n_extra == len(c.pi_other) and int(sources.max()) < n_words + n_extra
    assert len(set(cells.tolist())) == len(cells) and int(cells.max()) < c.num_wires * c.n
    # every extra word is used, and a probe proof whose word k holds k shows every source of the proof's part
    words, extra, pis = c.words_of_proof(o["proof"], data["caps"], data["points"], o["transcript"])
    assert set(sources[sources >= n_words].tolist()) == set(range(n_words, n_words + n_extra))
    staged = np.concatenate([words, extra])
    gcells, gvals, gpis = c.proof_inputs(o["proof"], data["caps"], data["points"], o["transcript"])
    assert (gcells == cells).all() and (staged[sources.astype(np.int64)] == gvals).all() and (pis == gpis).all()
    assert [int(v) for v in pis] == c.public_inputs(*o["args"][:6])


@pytest.mark.parametrize("routed, groups", [(80, (0, 0, 0, 0, 1, 1)), (67, (0, 0, 1, 1, 2, 2))])
def test_basic_is_satisfied_by_its_replayed_witness_and_proves(routed, groups):
    c = BasicCircuit(num_routed=routed, groups=groups)
    assert c.num_selectors == groups[-1] + 1 and sorted(set(c.gate[:c.rows_used].tolist())) == [1, 2, 3, 4, 5]
    cs = c.constants_sigmas()
    pis = c.public_inputs(PIS)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(c.partial_witness(PIS, INDEX), cs[:c.num_constants], c.generators(), pih, c.schedule())
    bits, out, claimed = c.expected(PIS, INDEX)
    assert [int(v) for v in w[1:5, c.split_row]] == bits and (int(w[6, c.arith_row]), int(w[7, c.arith_row])) == out
    assert int(w[1, c.ra_row]) == claimed == out[0] and [int(v) for v in w[0:4, c.pi_row]] == [int(v) for v in pih]
    o = {"c": c, "cs": cs}
    assert satisfied(o, w, pih) == ([], [])
    if routed == 80:                                            # prove_and_judge's parameters are R = 80
        o["cs_cap"] = _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap
        assert prove_and_judge(o, w, pis) == (0, 0)
    cells, vals = c.input_cells(PIS, INDEX)
    assert len(set(cells.tolist())) == len(cells) == sum(len(x) for x in c.pi_cycle + c.in_cycle)
