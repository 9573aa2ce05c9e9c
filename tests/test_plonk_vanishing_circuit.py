"""The vanishing equation of an outer proof in the outer circuit on the CPU (sipp_amd/plonk_vanishing.py): inner proofs by the oracle's
prover for the three inner circuits of tests/_plonk_vanishing_cases.py; the witness replayed level by level (tests/_witness_reading.py),
proved by the oracle and judged by both verifiers; every drawn and computed cell against the independent reading
(tests/_plonk_vanishing_reading.py), which itself stands against oracle/py/plonky2_generic.py and the library's verifier; the gate
compiler's counts; tampering; the refusals at build; the proof layout; PlonkProofVerifier's comparison of the pair; the pinned digests
of tests/golden/plonk_vanishing_shapes.json (tools/plonk_vanishing_shapes.py writes them)."""
import json
import os
import sys

import numpy as np
import pytest

from sipp_amd import fri_proof as fp
from sipp_amd import plonk_vanishing as pv
from tests import _challenger_reading  # noqa: F401  (registers the reading of generator kind 15, which the FRI circuit uses)
from tests import _oracle
from tests import _plonk_vanishing_cases as cases
from tests import _plonk_vanishing_reading as vr
from tests import _verify
from tests import _witness_reading as rd
from tests.test_fri_verifier_circuit import satisfied
from tests.test_oracle_plonk import fri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plonk_vanishing_shapes.json")
P = _oracle.P
DIGEST = (89, 90, 91, 92)                                       # of the outer circuits
OUTER = _oracle.plonk_params(80, 8, 2)
_built = {}


def build(name):
    """one case, once: the inner circuit and its proof by the oracle, the vanishing circuit, its arguments, the reading"""
    if name not in _built:
        o = cases.inner(name)
        pf = cases.oracle_proof(o)
        c = pv.PlonkVanishingCircuit(o["c"].log_n, o["params"], o["circ"], cases.CAP_HEIGHT, len(o["pis"]))
        cs = c.constants_sigmas()
        _built[name] = {"o": o, "proof": pf, "c": c, "cs": cs, "args": pv.flat_proof_arguments(c, pf, cases.INNER_DIGEST),
                        "reading": read(o, pf)}
    return _built[name]


def read(o, proof, digest=cases.INNER_DIGEST):
    return vr.read(proof, digest, o["c"].log_n, o["circ"], o["params"], cases.CAP_HEIGHT, len(o["pis"]))


def witness(b, args=None):
    """(the replayed witness, the public inputs, their hash); the good one of a case is kept"""
    if args is None:
        if "witness" not in b:
            b["witness"] = witness(b, b["args"])
        return b["witness"]
    c = b["c"]
    pis = c.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    return rd.replay(c.partial_witness(*args), b["cs"][:c.num_constants], c.generators(), pih, c.schedule()), pis, pih


@pytest.fixture(scope="module", params=cases.NAMES)
def whole(request):
    return build(request.param)


def test_the_inner_circuits_reach_what_they_are_for():
    basic, ragged, poseidon = (cases.inner(n) for n in cases.NAMES)
    assert basic["circ"]["num_selectors"] == 2 and basic["params"] == (80, 8, 2)
    assert ragged["circ"]["num_selectors"] == 1 and ragged["params"] == (67, 8, 1) and 67 % 8 == 3
    assert sorted(set(basic["c"].gate[:basic["c"].rows_used].tolist())) == [1, 2, 3, 4, 5]
    swap = [g for g, name in enumerate(poseidon["circ"]["gate_names"]) if name == "PoseidonSwap"][0]
    cons = pv.gate_constraints(poseidon["circ"], swap)
    words = [int(x) for x in poseidon["circ"]["programs"]]
    assert len(cons) == 123 and min(words) < 0 and any(kind == 2 for g in range(len(poseidon["circ"]["gates"]))
                                                       for monos in pv.gate_constraints(poseidon["circ"], g) for _, key in monos for kind, _ in key)
    assert max(len(key) for monos in cons for _, key in monos) == 7             # the S-box: x^7, its powers shared
    assert all(o["c"].log_n == 10 for o in (basic, ragged, poseidon))           # the smallest the FRI parameters admit


def test_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(whole):
    b, c = whole, whole["c"]
    o = b["o"]
    assert _oracle.plonk_verify_gates(b["proof"], o["cap"], o["op"], o["ofp"], o["circ"], cases.INNER_DIGEST) == 0
    w, pis, pih = witness(b)
    assert satisfied(b, w, pih) == ([], [])
    assert (w[12:16, c.chain_row[-1]] == pih).all() and [int(w.reshape(-1)[x]) for x in c.pi_cells] == pis
    ofp = fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    pf = _oracle.plonk_prove_gates(w, b["cs"], c.log_n, OUTER, ofp, c.circuit(), DIGEST, pis)
    cap = _oracle.Batch(b["cs"], c.log_n, rate_bits=3, cap_height=4).cap
    assert _oracle.plonk_verify_gates(pf, cap, OUTER, ofp, c.circuit(), DIGEST) == 0
    assert _verify.lib_plonk_verify(pf, cap, OUTER, ofp, c.circuit(), DIGEST) == 0


def test_the_cells_hold_the_readings_values(whole):
    b, c, r = whole, whole["c"], whole["reading"]
    w, pis, _ = witness(b)
    at = lambda cell: int(w[cell[0], cell[1]])
    ext = lambda cells: tuple(at(x) for x in cells)
    assert [at(x) for x in c.pih_cells] == r["pih"]
    assert [at(x) for x in c.beta_cells] == r["betas"] and [at(x) for x in c.gamma_cells] == r["gammas"]
    assert [at(x) for x in c.alpha_cells] == r["alphas"] and ext(c.zeta_cells) == r["zeta"]
    assert ext(c.zeta_n_cells) == r["zeta_n"] and ext(c.zh_cells) == r["zh"] and ext(c.l0_cells) == r["l0"]
    assert len(c.term_cells) == len(r["terms"]) == c.C + c.C * c.m + c.ngc
    assert [ext(t) for t in c.term_cells] == r["terms"]
    assert [(ext(x), ext(y)) for x, y in c.side_cells] == r["sides"] and all(x == y for x, y in r["sides"])
    assert ext(c.gzeta_cells) == r["gzeta"] and [at(x) for x in c.state_cells] == r["state"]
    # the outputs as public inputs, and the host transcript that hands them to the prover
    assert pis[c.pi_zeta:] == list(r["zeta"]) + list(r["gzeta"]) + r["state"]
    t = c.transcript(*b["args"][:3])
    assert all(t[k] == r[k] for k in ("pih", "betas", "gammas", "alphas", "zeta", "gzeta", "state"))


def test_the_reading_agrees_with_the_generic_oracle_and_the_librarys_verdict(whole):
    sys.path.insert(0, os.path.join(ROOT, "oracle", "py"))
    import plonky2_generic as g2
    b, r = whole, whole["reading"]
    o, s = b["o"], r["split"]
    R, D, C = o["params"]
    E = lambda v: g2.Ext(v[0], v[1])
    plain = lambda v: (int(v[0]), int(v[1]))
    # the transcript
    ch = g2.Challenger()
    ch.observe_many(list(cases.INNER_DIGEST) + [int(v) for v in g2.hash_no_pad(o["pis"])] + s["caps"][0])
    assert [ch.get() for _ in range(C)] == r["betas"] and [ch.get() for _ in range(C)] == r["gammas"]
    ch.observe_many(s["caps"][1])
    assert [ch.get() for _ in range(C)] == r["alphas"]
    ch.observe_many(s["caps"][2])
    assert (ch.get(), ch.get()) == r["zeta"]
    # the gate terms and the filters
    got = g2.evaluate_gate_constraints(o["circ"]["gates"], o["circ"]["programs"], o["circ"]["num_selectors"], [E(v) for v in s["wires"]],
                                       [E(v) for v in s["constants"]], r["pih"])
    assert [plain(v) for v in got] == r["terms"][C + C * -(-R // D):]
    for sel, row, lo, hi, _, _ in o["circ"]["gates"]:
        f = g2.compute_filter(row, range(lo, hi), E(s["constants"][sel]), o["circ"]["num_selectors"] > 1)
        want = vr.base(1)
        for i in list(range(lo, hi)) + ([0xFFFFFFFF] if o["circ"]["num_selectors"] > 1 else []):
            if i != row:
                want = vr.e_mul(want, vr.e_sub(vr.base(i), s["constants"][sel]))
        assert plain(f) == want
    # the verdict: the library's verifier accepts exactly when the reading's sides meet
    assert _verify.lib_plonk_verify(b["proof"], o["cap"], o["op"], o["ofp"], o["circ"], cases.INNER_DIGEST) == 0
    bad = b["proof"].copy()
    bad[s["opened_at"]] = (int(bad[s["opened_at"]]) + 1) % P
    assert _verify.lib_plonk_verify(bad, o["cap"], o["op"], o["ofp"], o["circ"], cases.INNER_DIGEST) == 210
    assert any(x != y for x, y in read(o, bad)["sides"])


def test_the_compiler_evaluates_every_distinct_monomial_once_and_fills_no_row_beyond_its_ops(whole):
    b, c = whole, whole["c"]
    circ = b["o"]["circ"]
    assert c.gate_monomials == [vr.distinct_monomials(circ, g) for g in range(len(circ["gates"]))]
    # products: one op per distinct monomial of two factors or more, at most (prefixes of a longer one that no constraint names add
    # theirs); sums: one op per monomial named
    named = sum(len(monos) for g in range(len(circ["gates"])) for monos in pv.gate_constraints(circ, g))
    keys = {key for g in range(len(circ["gates"])) for monos in pv.gate_constraints(circ, g) for _, key in monos}
    prefixes = {key[:k] for key in keys for k in range(2, len(key) + 1)}
    filters = sum(max(0, (hi - lo - 1) + (circ["num_selectors"] > 1) - 1) for _, _, lo, hi, _, _ in circ["gates"])
    factors = len({(sel, i) for sel, row, lo, hi, _, _ in circ["gates"] for i in list(range(lo, hi)) + [-1] * (circ["num_selectors"] > 1) if i != row})
    joins = sum(g[5] for g in circ["gates"])
    assert sum(c.gate_ops) <= named + len(prefixes) + filters + factors + joins
    assert sum(c.gate_ops) >= named + len({k for k in keys if len(k) >= 2})
    # rows: num_routed // 8 ops to a row at the most, every op in a row of the multi-op gate
    n_ops = c.num_routed // 8
    gens = {g[2]: g for g in c.generators()}
    assert n_ops == 10 and gens[pv.ARITHMETIC_EXT][3] == n_ops and 8 * n_ops <= c.num_routed and gens[pv.QUOTIENT_EXT][3] == 1
    assert all(c.gate[r] == pv.ARITHMETIC_EXT for r in c.ops.rows) and len(set(c.ops.rows)) == len(c.ops.rows)
    flat = {x for cyc in c.cycles + c.pi_cycle for x in cyc}
    for r in c.ops.rows:                                        # no cell behind the row's ops is wired
        assert not any((wire * c.n + r) in flat for wire in range(8 * n_ops, c.num_routed))
    assert c.ops.count <= n_ops * len(c.ops.rows)


def test_every_filtered_constraint_of_the_outer_circuit_has_degree_at_most_8(whole):
    circ = whole["c"].circuit()
    for g, (sel, row, lo, hi, _, _) in enumerate(circ["gates"]):
        degree = max((len(key) for monos in pv.gate_constraints(circ, g) for _, key in monos), default=0)
        assert (hi - lo - 1) + (circ["num_selectors"] > 1) + degree <= 8, circ["gate_names"][g]


# ---- tampering: one word each -------------------------------------------------------------------------------------------------------
TAMPERS = ("constant", "sigma", "wire", "z", "partial_product", "quotient", "z_next", "wires_cap", "z_cap", "quotient_cap", "public_input",
           "digest")


def tampered(b, what):
    """(the inner proof, the digest) with one word changed"""
    c, pf, digest = b["c"], b["proof"].copy(), list(cases.INNER_DIGEST)
    opened_at = 16 + 12 * c.n_cap + 8
    first = {"constant": 0, "sigma": c.K, "wire": c.K + c.R, "z": c.K + c.R + c.W, "partial_product": c.K + c.R + c.W + c.C,
             "quotient": c.K + c.R + c.W + c.nz, "z_next": c.n0}
    if what in first:
        at = opened_at + 2 * first[what] + 1                    # limb 1 of the first value of its kind
    elif what.endswith("_cap"):
        at = 16 + 4 * c.n_cap * ("wires_cap", "z_cap", "quotient_cap").index(what) + 5
    elif what == "public_input":
        at = len(pf) - 2
    else:
        digest[2] += 1
        return pf, digest
    pf[at] = (int(pf[at]) + 1) % P
    return pf, digest


@pytest.mark.parametrize("what", TAMPERS)
def test_one_tampered_word_breaks_only_the_closing_ties(what):
    b = build("ragged")
    c, o = b["c"], b["o"]
    pf, digest = tampered(b, what)
    assert any(x != y for x, y in read(o, pf, digest)["sides"])
    assert _oracle.plonk_verify_gates(pf, o["cap"], o["op"], o["ofp"], o["circ"], digest) == -210
    w, pis, pih = witness(b, pv.flat_proof_arguments(c, pf, digest))
    rows, cycles = satisfied(b, w, pih)
    cell = lambda x: x[0] * c.n + x[1]
    ties = {cell(x) for sides in c.side_cells for side in sides for x in side}
    assert rows == [] and cycles and all(ties & set(cyc) for cyc in cycles)


# ---- the refusals at build ----------------------------------------------------------------------------------------------------------
def test_refusals_at_build():
    o = cases.inner("ragged")
    args = lambda **kw: dict(dict(log_n=10, params=(67, 8, 1), circuit=o["circ"], cap_height=4, n_pi_inner=5), **kw)
    with pytest.raises(AssertionError, match="public inputs"):
        pv.PlonkVanishingCircuit(**args(n_pi_inner=0))
    with pytest.raises(AssertionError, match="8 challenges"):
        pv.PlonkVanishingCircuit(**args(params=(67, 8, 9)))
    with pytest.raises(AssertionError, match="power of two"):
        pv.PlonkVanishingCircuit(**args(params=(67, 6, 1)))
    words = o["circ"]["programs"].copy()
    words[3] = 3                                                # a factor kind nobody knows
    for bad in (dict(o["circ"], programs=o["circ"]["programs"][:-3]), dict(o["circ"], programs=words), dict(o["circ"], num_selectors=0),
                dict(o["circ"], num_wires=66)):
        with pytest.raises(AssertionError, match="refused"):
            pv.PlonkVanishingCircuit(**args(circuit=bad))
        assert _refused_by_the_library(bad, o)


def _refused_by_the_library(circ, o):
    """sipp_plonk_verify_gates answers 201 for a gate set circuit_ok refuses"""
    try:
        return _verify.lib_plonk_verify(cases.oracle_proof(o), o["cap"], o["op"], o["ofp"], circ, cases.INNER_DIGEST) == 201
    except Exception:                                           # a dict the binding itself cannot take
        return True


# ---- the flat proof ---------------------------------------------------------------------------------------------------------------------
def test_proof_layout_is_input_cells(whole):
    b, c = whole, whole["c"]
    cells, words, pi_word = c.proof_layout(len(b["proof"]))
    staged = np.concatenate([b["proof"], np.array(cases.INNER_DIGEST, dtype=np.uint64)])
    gcells, gvals = c.input_cells(*b["args"])
    assert cells.dtype == words.dtype == np.uint64 and (cells == gcells).all() and (staged[words.astype(np.int64)] == gvals).all()
    assert len(set(cells.tolist())) == len(cells) and int(words.max()) < len(staged)
    pis = c.public_inputs(*b["args"])
    assert [int(v) for v in staged[pi_word[:c.pi_zeta]]] == pis[:c.pi_zeta] and (pi_word[c.pi_zeta:] == -1).all()
    # the outputs' cells are generated: no input cell is one of them
    out = {x for t in range(c.pi_zeta, c.n_pi) for x in c.pi_cycle[t]}
    assert not out & set(cells.tolist())


# ---- the pair -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """ragged: both outer proofs by the oracle, and the verifying half of PlonkProofVerifier built without a device"""
    from tests.test_gpu_fri_generic import to_params
    b = build("ragged")
    o, v = b["o"], b["c"]
    w, pis, _ = witness(b)
    ofp = fri(v.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    first = _oracle.plonk_prove_gates(w, b["cs"], v.log_n, OUTER, ofp, v.circuit(), DIGEST, pis)
    K, W, (R, D, C) = v.K, v.W, o["params"]
    f = fp.FriProofCircuit(v.inner_log_n + 3, 4, [K + R, W, v.nz, C * D], [list(range(v.n0)), list(range(K + R + W, K + R + W + C))], 4, 2,
                           (1 << v.inner_log_n) >> 8, 8, pow_bits=o["ofp"].pow_bits, pow_rule=0, n_in=0)
    section = b["proof"][16 + 12 * v.n_cap:len(b["proof"]) - len(o["pis"])]
    caps = [o["cap"].reshape(-1)] + [b["proof"][16 + 4 * v.n_cap * k:16 + 4 * v.n_cap * (k + 1)] for k in range(3)]
    r = b["reading"]
    args = fp.flat_proof_arguments(f, section, caps, [r["zeta"], r["gzeta"]], (r["state"], []))
    fpis = f.public_inputs(*args[:6])
    fcs = f.constants_sigmas()
    fpih = _oracle.hash_no_pad(np.array(fpis, dtype=np.uint64))
    fw = rd.replay(f.partial_witness(*args), fcs[:f.num_constants], f.generators(), fpih, f.schedule())
    assert satisfied({"c": f, "cs": fcs}, fw, fpih) == ([], [])
    ffp = fri(f.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    assert f.log_n == v.log_n + 1
    second = _oracle.plonk_prove_gates(fw, fcs, f.log_n, OUTER, ffp, f.circuit(), DIGEST, fpis)
    data = [(_oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap, DIGEST) for cs, c in ((b["cs"], v), (fcs, f))]
    return b, (first, second), data, to_params(ofp), to_params(ffp), to_params(o["ofp"])


def test_the_pair_is_accepted_and_every_difference_is_refused(pair):
    b, (first, second), data, gfp_v, gfp_f, inner_fri = pair
    o = b["o"]
    ver = pv.PlonkProofVerifier(None, o["c"].log_n, o["params"], o["circ"], inner_fri, len(o["pis"]), fri=(gfp_v, gfp_f), verifier_data=data)
    assert ver.verify((first, second), o["cap"], cases.INNER_DIGEST) == o["pis"]
    v, f = ver.vc, ver.fc
    # one word per class of shared public inputs, in either proof: the proof itself no longer verifies, or the comparison refuses
    n1, n2 = len(first) - v.n_pi, len(second) - f.n_pi
    spots = {"state": (n1 + v.pi_state + 3, n2 + 3), "zeta": (n1 + v.pi_zeta, n2 + f.pi_batch[0]), "gzeta": (n1 + v.pi_gzeta + 1, n2 + f.pi_batch[1] + 1),
             "opened": (n1 + v.pi_opened + 9, n2 + f.pi_batch[0] + 2 + 9), "opened_next": (n1 + v.pi_opened + 2 * v.n0, n2 + f.pi_batch[1] + 2),
             "caps": (n1 + v.pi_caps + 6, n2 + f.pi_caps + 4 * v.n_cap + 6)}
    for what, (a1, a2) in spots.items():
        for k, at in enumerate((a1, a2)):
            bad = [first.copy(), second.copy()]
            bad[k][at] = (int(bad[k][at]) + 1) % P
            assert [w_ for w_, x, y in ver.shared(bad) if x != y] == [what]
            with pytest.raises(ValueError):
                ver.verify(bad, o["cap"], cases.INNER_DIGEST)
    # the comparison alone, with proofs that verify: another cap, another digest
    wrong_cap = o["cap"].copy()
    wrong_cap[0, 0] ^= np.uint64(1)
    with pytest.raises(ValueError, match="constants_sigmas cap"):
        ver.verify((first, second), wrong_cap, cases.INNER_DIGEST)
    with pytest.raises(ValueError, match="digest"):
        ver.verify((first, second), o["cap"], (21, 22, 23, 25))


# ---- the pinned shapes ------------------------------------------------------------------------------------------------------------------
def shape_digests(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import outer_circuit_shapes as shapes
    b = build(name)
    return shapes.digests(b["c"], b["args"], b["args"])


@pytest.mark.parametrize("name", cases.NAMES)
def test_shape_is_the_pinned_one(name):
    want = json.load(open(GOLDEN))[name]
    got = shape_digests(name)
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []
