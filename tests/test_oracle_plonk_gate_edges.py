"""The outer prover's gate programs at their edges (tests/_gate_edges.py), three readings on the CPU: per row, the exact Python-integer
evaluation of the programs, oracle/plonk_gates.c and oracle/py/plonky2_generic.py agree (and vanish on satisfied rows); the oracle's proof of
every catalogue circuit gets the same verdict from the oracle's verifier, the library's verify.cpp (sipp_plonk_verify_gates, host code)
and the Python replay at zeta; what both verifiers say about the circuits at and beyond the prover's limits."""
import pytest

from oracle.py import plonky2_generic as g2
from tests import _gate_edges as ge
from tests import _oracle, _verify

P = _oracle.P
DIGEST = (17, 0, P - 1, 1 << 32)

ENTRIES = [f for _, f in ge.ENTRIES]
IDS = [name for name, _ in ge.ENTRIES]


def cs_cap(entry):
    return _oracle.Batch(entry["cs"], entry["log_n"], rate_bits=ge.FRI["rate_bits"], cap_height=ge.FRI["cap_height"]).cap


def verdicts(pf, entry):
    """(oracle, verify.cpp, python replay per challenge)"""
    p, fp, circ = ge.params(entry), ge.fri_params(entry), entry["circ"]
    cap = cs_cap(entry)
    return (_oracle.plonk_verify_gates(pf, cap, p, fp, circ, DIGEST), _verify.lib_plonk_verify(pf, cap, p, fp, circ, DIGEST),
            _verify.py_plonk_replay(pf, circ, p, fp, DIGEST, entry["pis"]))


def assert_verdicts(pf, entry):
    orc, lib, py = verdicts(pf, entry)
    if entry["accept"]:
        assert (orc, lib, py) == (0, 0, [True] * entry["num_challenges"]), entry["name"]
    else:
        assert orc == -210 and lib == 210 and not all(py), (entry["name"], orc, lib, py)


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_three_readings_agree_on_every_row(make):
    """per row: exact evaluation (filter included) == oracle/plonk_gates.c (base field) == plonky2_generic over the extension with base
    inputs; zero on every satisfied row, not zero on a tampered one"""
    e = make()
    circ, K, ngc = e["circ"], e["circ"]["num_constants"], e["circ"]["num_gate_constraints"]
    for r in range(1 << e["log_n"]):
        wires = [int(x) for x in e["wires"][:, r]]
        consts = [int(x) for x in e["cs"][:K, r]]
        exact = ge.eval_row_exact(circ, wires, consts, e["pih"])
        orc = [int(x) for x in _oracle.plonk_gate_constraints_base(circ, e["wires"][:, r], e["cs"][:K, r], e["pih"])][:ngc]
        py = g2.evaluate_gate_constraints(circ["gates"], circ["programs"], circ["num_selectors"], [g2.ext(v) for v in wires],
                                          [g2.ext(v) for v in consts], e["pih"])
        assert orc == exact, (e["name"], r)
        assert [int(v[0]) for v in py] == exact and all(int(v[1]) == 0 for v in py), (e["name"], r)
        assert any(exact) == (r in e["bad_rows"]), (e["name"], r, int(e["gate"][r]))


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_oracle_proof_through_every_verifier(make):
    """the oracle's proof: accepted by all three readings on satisfied circuits, refused at the quotient identity (stage 210) by all three
    on the over-degree and tampered ones"""
    e = make()
    pf = _oracle.plonk_prove_gates(e["wires"], e["cs"], e["log_n"], ge.params(e), ge.fri_params(e), e["circ"], DIGEST, e["pis"])
    assert int(pf[10]) == e["circ"]["num_gate_constraints"] and int(pf[8]) == e["circ"]["num_selectors"]
    assert_verdicts(pf, e)


def test_the_edges_are_in_the_catalogue():
    """the programs really contain what the catalogue claims: one selector column; nf = 0; n_mono = 0; a gate of empty constraints; a
    circuit without gate constraints; duplicates; every int64 edge as a coefficient; 4 .. 8 challenges; groups of 1 and 64 gates; 64-factor
    pure and mixed monomials; 4096 monomials; operands at the last index of each kind"""
    def monos(circ):
        prog, out = [int(x) for x in circ["programs"]], []
        for (_s, _r, _lo, _hi, off, nc) in circ["gates"]:
            w = off
            for j in range(nc):
                nm, w = prog[w], w + 1
                out.append((nm, []))
                for _ in range(nm):
                    coef, nf = prog[w], prog[w + 1]
                    out[-1][1].append((coef, [tuple(prog[w + 2 + 2 * q:w + 4 + 2 * q]) for q in range(nf)]))
                    w += 2 + 2 * nf
        return out
    cat = {e["name"]: e for e in ge.catalogue()}
    ss, rich, ms = monos(cat["single_selector"]["circ"]), monos(cat["rich"]["circ"]), monos(cat["many_monomials"]["circ"])
    assert cat["single_selector"]["circ"]["num_selectors"] == 1 and cat["group64"]["circ"]["num_selectors"] == 1
    assert any(not f for _, ms_ in ss for _, f in ms_) and any(nm == 0 for nm, _ in ss)
    assert any(g[5] > 0 and all(nm == 0 for nm, _ in monos(dict(cat["single_selector"]["circ"], gates=[g]))) for g in cat["single_selector"]["circ"]["gates"])
    assert cat["no_gate_constraints"]["circ"]["num_gate_constraints"] == 0
    coefs = {c for _, m in ss for c, _ in m}
    assert set(ge.EDGE_COEFS) <= coefs
    for mono_list in (ss, rich):
        sorted_sets = [sorted(f) for _, m in mono_list for _, f in m]
        assert any(sorted(f) != f and sorted(f) in sorted_sets for _, m in mono_list for _, f in m)     # another factor order
    assert {e["num_challenges"] for e in ge.catalogue()} >= {1, 2, 3, 4, 6, 7, 8}
    assert {g[3] - g[2] for g in cat["rich"]["circ"]["gates"]} >= {1, 2, 3} and {g[3] - g[2] for g in cat["group64"]["circ"]["gates"]} == {64}
    nfs = [len(f) for _, m in monos(cat["pow64"]["circ"]) for _, f in m]
    assert nfs.count(64) == 3 and max(nfs) == 64
    assert max(nm for nm, _ in ms) == 4096
    # the pure-power order compile_gates gives a gate (distinct monomials, by operand then exponent): neighbours where the chained product
    # must not fire (next index, other kind, a gap) and where it must
    pairs = set()
    for e in (cat["single_selector"], cat["rich"]):
        for g in e["circ"]["gates"]:
            pure = sorted({(f[0], len(f)) for _, m in monos(dict(e["circ"], gates=[g])) for _, f in m if f and len(set(f)) == 1})
            for (a, x), (b, y) in zip(pure, pure[1:]):
                pairs.add("chain" if a == b and y == x + 1 else "gap" if a == b else "next index" if a[0] == b[0] and y == x + 1 else
                          "other kind" if a[1] == b[1] and y == x + 1 else "other")
    assert {"chain", "gap", "next index", "other kind"} <= pairs
    ops = {op for _, m in ms for _, f in m for op in f}
    circ = cat["many_monomials"]["circ"]
    assert {(0, circ["num_wires"] - 1), (1, circ["num_constants"] - 1), (2, 3)} <= ops


@pytest.mark.parametrize("limit", range(len(ge.LIMIT_IDS)), ids=ge.LIMIT_IDS)
def test_verifiers_at_the_prover_limits(limit):
    """the circuits at and one step beyond each limit of the prover's circuit_check, through the oracle (prover and verifier) and
    verify.cpp.  Just inside: the oracle proves; the over-degree circuits are refused at 210, the others accepted.  Just outside: the
    oracle's prover takes a 65-gate group (refused at 210 by both verifiers: over-degree) and 4097 wires, 1025 constants or 4097
    constraints (accepted by both: they share none of these limits); a 65-factor monomial, 4097 monomials or an operand past the last
    index is malformed for the oracle's prover (-1) and for both verifiers (-201 / 201)"""
    name, inside, outside, outside_entry = ge.limits()[limit]
    p, fp = ge.params(inside), ge.fri_params(inside)
    pf = _oracle.plonk_prove_gates(inside["wires"], inside["cs"], inside["log_n"], p, fp, inside["circ"], DIGEST, inside["pis"])
    assert_verdicts(pf, inside)
    if outside_entry is not None:
        e = outside_entry
        assert e["circ"] is outside
        assert_verdicts(_oracle.plonk_prove_gates(e["wires"], e["cs"], e["log_n"], p, fp, outside, DIGEST, e["pis"]), e)
    else:
        with pytest.raises(RuntimeError):
            _oracle.plonk_prove_gates(inside["wires"], inside["cs"], inside["log_n"], p, fp, outside, DIGEST, inside["pis"])
        cap = cs_cap(inside)
        assert _oracle.plonk_verify_gates(pf, cap, p, fp, outside, DIGEST) == -201
        assert _verify.lib_plonk_verify(pf, cap, p, fp, outside, DIGEST) == 201
