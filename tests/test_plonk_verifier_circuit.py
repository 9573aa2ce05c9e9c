"""plonky2's verify as ONE outer circuit on the CPU (sipp_amd/plonk_verifier.py): inner proofs by the oracle's prover for the inner
circuits of tests/_plonk_vanishing_cases.py (the Poseidon one with poseidon_mds=True, alpha_chunk=8 and with the defaults); the witness
replayed level by level (tests/_witness_reading.py), proved by the oracle, judged by both verifiers; the drawn and computed cells
against the readings of both halves (tests/_plonk_vanishing_reading.py, tests/_challenger_reading.py); the counted conditions of the
join; one tampered word per class; a proof spliced from two; the refusals at build; the verifying half without a device; the pinned
shapes of tests/golden/plonk_verifier_shapes.json (tools/plonk_verifier_shapes.py writes them)."""
import json
import os
import sys

import numpy as np
import pytest

from sipp_amd import fri_proof as fp
from sipp_amd import plonk_vanishing as pv
from sipp_amd import plonk_verifier as pj
from tests import _challenger_reading as cr
from tests import _oracle
from tests import _plonk_vanishing_cases as cases
from tests import _poseidon_mds_reading  # noqa: F401  (registers the reading of generator kind 16)
from tests import _verify
from tests import _witness_reading as rd
from tests.test_fri_verifier_circuit import satisfied
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri
from tests.test_plonk_vanishing_circuit import TAMPERS, read, tampered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plonk_verifier_shapes.json")
P = _oracle.P
DIGEST = (89, 90, 91, 92)                                       # of the outer circuit
OUTER = _oracle.plonk_params(80, 8, 2)
# case -> (the inner circuit, the joined circuit's keywords, its generator count)
CASES = {"basic": ("basic", {}, 16), "ragged": ("ragged", {}, 16), "poseidon": ("poseidon", {}, 16),
         "poseidon-mds": ("poseidon", dict(poseidon_mds=True, alpha_chunk=8), 17)}
_built = {}


def outer_fri(c):
    return fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)


def shape(o):
    return (o["c"].log_n, o["params"], o["circ"], to_params(o["ofp"]), len(o["pis"]))


def build(case):
    if case not in _built:
        inner, kw, _ = CASES[case]
        o = cases.inner(inner)
        pf = cases.oracle_proof(o)
        c = pj.PlonkVerifierCircuit(*shape(o), **kw)
        _built[case] = {"o": o, "proof": pf, "c": c, "kw": kw, "cs": c.constants_sigmas(),
                        "args": pj.flat_proof_arguments(c, pf, o["cap"], cases.INNER_DIGEST)}
    return _built[case]


def witness(b, args=None):
    """(the replayed witness, the public inputs, their hash); the good one of a case is kept"""
    if args is None:
        if "witness" not in b:
            b["witness"] = witness(b, b["args"])
        return b["witness"]
    c = b["c"]
    pis = c.public_inputs(*args[:3])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    return rd.replay(c.partial_witness(*args), b["cs"][:c.num_constants], c.generators(), pih, c.schedule()), pis, pih


def outer_proof(b):
    """the good witness proved by the oracle, once -> (the proof, the outer circuit's constants_sigmas cap)"""
    if "outer" not in b:
        c = b["c"]
        w, pis, _ = witness(b)
        b["outer"] = (_oracle.plonk_prove_gates(w, b["cs"], c.log_n, OUTER, outer_fri(c), c.circuit(), DIGEST, pis),
                      _oracle.Batch(b["cs"], c.log_n, rate_bits=3, cap_height=4).cap)
    return b["outer"]


def second_inner_inputs(o):
    """another statement of the same inner circuit, as tests/test_gpu_plonk_vanishing_circuit.py makes for its stitched pairs: other
    public inputs (basic, ragged) or another leaf (poseidon) -> (the public inputs, the partial witness)"""
    c = o["c"]
    if o["name"] == "poseidon":
        from oracle.py import plonky2_generic as g2
        leaves = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 17]]
        tree = g2.MerkleTree(leaves, 1)
        args = ([v for d in tree.cap for v in d], [3], [leaves[3]], [tree.prove(3)])
        return [int(v) for v in c.public_inputs(*args[:3])], c.partial_witness(*args)
    args = ([6, 1, 2, 3, 4], 1)
    return [int(v) for v in c.public_inputs(args[0])], c.partial_witness(*args)


def second_inner_proof(o):
    """that statement's proof by the oracle -> (the proof, its public inputs)"""
    c = o["c"]
    pis, pw = second_inner_inputs(o)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(pw, o["cs"][:c.num_constants], c.generators(), pih, c.schedule())
    return _oracle.plonk_prove_gates(w, o["cs"], c.log_n, o["op"], o["ofp"], o["circ"], cases.INNER_DIGEST, pis), pis


@pytest.fixture(scope="module", params=sorted(CASES))
def whole(request):
    return build(request.param)


def test_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(whole):
    b, c = whole, whole["c"]
    w, pis, pih = witness(b)
    assert satisfied(b, w, pih) == ([], [])
    assert (w[12:16, c.chain_row[-1]] == pih).all() and [int(w.reshape(-1)[x]) for x in c.pi_cells] == pis
    pf, cap = outer_proof(b)
    assert _oracle.plonk_verify_gates(pf, cap, OUTER, outer_fri(c), c.circuit(), DIGEST) == 0
    assert _verify.lib_plonk_verify(pf, cap, OUTER, outer_fri(c), c.circuit(), DIGEST) == 0


def test_the_cells_hold_the_readings_values(whole):
    b, c, o = whole, whole["c"], whole["o"]
    w, _, _ = witness(b)
    at = lambda cell: int(w[cell[0], cell[1]])
    ext = lambda cells: tuple(at(x) for x in cells)
    # the vanishing half
    r = read(o, b["proof"])
    assert [at(x) for x in c.pih_cells] == r["pih"] and [at(x) for x in c.plonk_beta_cells] == r["betas"]
    assert [at(x) for x in c.plonk_gamma_cells] == r["gammas"] and [at(x) for x in c.plonk_alpha_cells] == r["alphas"]
    assert ext(c.zeta_cells) == r["zeta"] and ext(c.gzeta_cells) == r["gzeta"] and [at(x) for x in c.state_cells] == r["state"]
    assert [ext(t) for t in c.term_cells] == r["terms"] and len(r["terms"]) == c.C + c.C * c.m + c.ngc
    assert [(ext(x), ext(y)) for x, y in c.side_cells] == r["sides"] and all(x == y for x, y in r["sides"])
    # the FRI half: what the challenger that leaves the vanishing half draws from the opening section
    section = b["proof"][c.section_at:len(b["proof"]) - c.n_pi_inner]
    d = cr.drawn(section, (r["state"], []), c.log_m, c.cap_height, c.n_open, c.arity_bits, c.n_rounds, c.final_len, c.n_queries, c.pow_rule)
    assert ext(c.alpha_cells) == d["alpha"] and [ext(x) for x in c.beta_cells] == d["betas"]
    assert at(c.response_cell) == d["response"] and [at(x) for x in c.index_cells] == d["challenges"]
    assert [sum(at((1 + i, c.bs_row[q])) << i for i in range(c.log_m)) for q in range(c.n_queries)] == d["x_index"]


def test_counted_conditions_of_the_join(whole):
    b, c, o = whole, whole["c"], whole["o"]
    n_pi_inner, n_cap = len(o["pis"]), 1 << cases.CAP_HEIGHT
    assert c.n_pi == 4 + n_pi_inner + 4 * n_cap and len(b["proof"]) == c.proof_words
    # every proof word that is no header word and no inner public input is the source of exactly one witness input, and no witness
    # input is without a word
    headers = set(range(pv.HEADER_WORDS)) | set(range(c.section_at, c.section_at + fp.HEADER_WORDS))
    inner_pi_words = set(range(c.proof_words - n_pi_inner, c.proof_words))
    words = [c.word_of[key] for key in c._in_keys]
    assert len(words) == len(c.in_cycle) == len(set(words)) and all(len(cyc) >= 1 for cyc in c.in_cycle)
    assert set(words) == set(range(c.proof_words)) - headers - inner_pi_words
    # the public inputs come from the inner public inputs and from extra = digest || constants_sigmas cap
    assert sorted(int(x) for x in c.pi_word) == sorted(list(inner_pi_words) + list(range(c.proof_words, c.proof_words + 4 + 4 * n_cap)))
    # the input map is the input cells, every cell once
    cells, sources = c.input_map(len(b["proof"]))
    staged = np.concatenate(c.words_of_proof(b["proof"], o["cap"], cases.INNER_DIGEST)[:2])
    gcells, gvals = c.input_cells(*b["args"])
    assert cells.dtype == sources.dtype == np.uint64 and (cells == gcells).all() and (staged[sources.astype(np.int64)] == gvals).all()
    assert len(set(cells.tolist())) == len(cells) and c.words_map()[2:] == (c.proof_words, 4 + 4 * n_cap)
    # fewer rows than the two circuits PlonkProofVerifier builds
    ver = pv.PlonkProofVerifier(None, *shape(o), fri=(to_params(outer_fri(c)),) * 2, verifier_data=[(o["cap"], DIGEST)] * 2, **b["kw"])
    assert c.rows_used < ver.vc.rows_used + ver.fc.rows_used
    # every filtered constraint has degree <= 8
    circ = c.circuit()
    for g, (sel, row, lo, hi, _, _) in enumerate(circ["gates"]):
        degree = max((len(key) for monos in pv.gate_constraints(circ, g) for _, key in monos), default=0)
        assert (hi - lo - 1) + (circ["num_selectors"] > 1) + degree <= 8, circ["gate_names"][g]


@pytest.mark.parametrize("case", sorted(CASES))
def test_generator_count(case):
    c = build(case)["c"]
    assert len(c.generators()) == CASES[case][2] and (len(c.generators()) > 16) == bool(c.poseidon_mds)


# ---- tampering: one word each -------------------------------------------------------------------------------------------------------
SECTION_TAMPERS = {"sibling": ("sibling", 2, 1, 3, 0), "evaluation": ("eval", 0, 0, 5, 1), "final_coefficient": ("final", 1, 1),
                   "pow_witness": ("pow_witness",), "round_cap": ("round_cap", 0, 3, 1)}


def tampered_proof(b, what):
    """(the inner proof, the digest) with one word changed: the classes of tests/test_plonk_vanishing_circuit.py and the opening
    section's"""
    if what in TAMPERS:
        return tampered(b, what)
    pf = b["proof"].copy()
    at = b["c"].word_of[SECTION_TAMPERS[what]]
    pf[at] = (int(pf[at]) + 1) % P
    return pf, list(cases.INNER_DIGEST)


@pytest.mark.parametrize("what", TAMPERS + tuple(sorted(SECTION_TAMPERS)))
def test_one_tampered_word_breaks_a_tie_or_a_constraint(what):
    b = build("ragged")
    c, o = b["c"], b["o"]
    pf, digest = tampered_proof(b, what)
    assert _oracle.plonk_verify_gates(pf, o["cap"], o["op"], o["ofp"], o["circ"], digest) != 0
    w, _, pih = witness(b, pj.flat_proof_arguments(c, pf, o["cap"], digest))
    assert satisfied(b, w, pih) != ([], [])


@pytest.mark.parametrize("case", ["ragged", "poseidon-mds"])
def test_a_proof_spliced_from_two_is_not_satisfied(case):
    """the caps and opened values of proof B (its public inputs with them: the vanishing half holds) with the rest of proof A's
    opening section: PlonkProofVerifier needed its host comparison to notice such a pair"""
    b = build(case)
    c, o = b["c"], b["o"]
    other, pis = second_inner_proof(o)
    assert _oracle.plonk_verify_gates(other, o["cap"], o["op"], o["ofp"], o["circ"], cases.INNER_DIGEST) == 0 and pis != o["pis"]
    rest = c.word_of["opened", c.n_open - 1, 1] + 1
    spliced = other.copy()
    spliced[rest:len(spliced) - c.n_pi_inner] = b["proof"][rest:len(spliced) - c.n_pi_inner]
    r = read(o, spliced)
    assert all(x == y for x, y in r["sides"])                   # the vanishing equation alone does not notice
    w, _, pih = witness(b, pj.flat_proof_arguments(c, spliced, o["cap"], cases.INNER_DIGEST))
    assert satisfied(b, w, pih) != ([], [])
    w, _, pih = witness(b, pj.flat_proof_arguments(c, other, o["cap"], cases.INNER_DIGEST))
    assert satisfied(b, w, pih) == ([], [])


# ---- the refusals at build ----------------------------------------------------------------------------------------------------------
def test_refusals_at_build():
    o = cases.inner("ragged")

    def refused(match, inner_fri=None, **kw):
        f = to_params(o["ofp"])
        for name, v in (inner_fri or {}).items():
            if name == "arity_bits":
                for r, a in enumerate(v):
                    f.arity_bits[r] = a
            else:
                setattr(f, name, v)
        args = dict(dict(log_n=10, params=(67, 8, 1), circuit=o["circ"], inner_fri=f, n_pi_inner=5), **kw)
        with pytest.raises(AssertionError, match=match):
            pj.PlonkVerifierCircuit(**args)
    refused("public inputs", n_pi_inner=0)
    refused("8 challenges", params=(67, 8, 9))
    refused("power of two", params=(67, 6, 1))
    refused("refused", circuit=dict(o["circ"], num_selectors=0))
    refused("poseidon_mds", poseidon_mds=True)
    refused("alpha_chunk", alpha_chunk=1)
    refused("cap height", inner_fri={"cap_height": 7})
    refused("cap height", inner_fri={"cap_height": 0})
    refused("mixed arities", inner_fri={"arity_bits": (4, 2)})
    refused("salted", inner_fri={"hiding": 1})
    refused("32 bits", inner_fri={"pow_bits": 33})


# ---- the verifying half without a device --------------------------------------------------------------------------------------------
def test_verify_without_a_device():
    b = build("ragged")
    c, o = b["c"], b["o"]
    pf, cap = outer_proof(b)
    ver = pj.PlonkVerifierProver(None, *shape(o), fri=to_params(outer_fri(c)), verifier_data=(cap, DIGEST))
    assert ver.verify(pf, o["cap"], cases.INNER_DIGEST) == o["pis"] and ver.verify(pf) == (0, 0)
    wrong_cap = o["cap"].copy()
    wrong_cap[0, 0] ^= np.uint64(1)
    with pytest.raises(ValueError, match="constants_sigmas cap"):
        ver.verify(pf, wrong_cap, cases.INNER_DIGEST)
    with pytest.raises(ValueError, match="digest"):
        ver.verify(pf, o["cap"], (21, 22, 23, 25))
    bad = pf.copy()
    bad[len(bad) - c.n_pi + c.pi_inner + 1] = (int(bad[len(bad) - c.n_pi + c.pi_inner + 1]) + 1) % P
    with pytest.raises(ValueError, match="refused: status"):
        ver.verify(bad, o["cap"], cases.INNER_DIGEST)
    ver.close()


# ---- the pinned shapes ------------------------------------------------------------------------------------------------------------------
def shape_digests(case):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import outer_circuit_shapes as shapes
    b = build(case)
    c = b["c"]
    out = shapes.digests(c, b["args"], b["args"][:3])
    out.update(rows_used=c.rows_used, log_n=c.log_n, n_levels=c.n_levels, n_public_inputs=c.n_pi, n_witness_inputs=len(c.in_cycle),
               n_input_cells=len(c.input_map()[0]), n_generators=len(c.generators()))
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_shape_is_the_pinned_one(case):
    want = json.load(open(GOLDEN))[case]
    got = shape_digests(case)
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []
