"""The inner Poseidon gate through MDS rows, and the closing Horner in chunks, on the CPU (sipp_amd/plonk_vanishing.py with poseidon_mds
and alpha_chunk; sipp_amd/merkle.py's poseidon_mds_gate): the gate program on rows written by the reading of kind 16
(tests/_poseidon_mds_reading.py), non-canonical inputs included; the `poseidon` case of tests/_plonk_vanishing_cases.py under the route,
under chunks of 8 and under both, and `basic` under chunks of 8 (a ragged last chunk) and under one chunk -- the witness replayed with
the readings, every row and cycle satisfied, every term and side cell against tests/_plonk_vanishing_reading.read, the outer proof by
the oracle judged by both verifiers; the counted shape conditions for two inner circuits, with the exact counts and digests pinned in
tests/golden/plonk_vanishing_mds_shapes.json (tools/outer_circuit_shapes.py --mds writes it); tampering; the refusals at build; the
pair of PlonkProofVerifier under both keywords, and a pair whose vanishing proof came from the default circuit."""
import json
import os
import sys

import numpy as np
import pytest

from sipp_amd import fri_proof as fp
from sipp_amd import merkle as mk
from sipp_amd import plonk_vanishing as pv
from sipp_amd.circuit import SWAP_LAYOUT
from tests import _challenger_reading  # noqa: F401  (registers the reading of generator kind 15, which the FRI circuit uses)
from tests import _oracle
from tests import _plonk_vanishing_cases as cases
from tests import _plonk_vanishing_reading as vr
from tests import _poseidon_mds_reading as pm
from tests import _verify
from tests import _witness_reading as rd
from tests.test_fri_verifier_circuit import satisfied
from tests.test_oracle_plonk import fri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plonk_vanishing_mds_shapes.json")
P = _oracle.P
DIGEST = (89, 90, 91, 92)                                       # of the outer circuits
OUTER = _oracle.plonk_params(80, 8, 2)
ROUTE, CHUNKS, BOTH = dict(poseidon_mds=True), dict(alpha_chunk=8), dict(poseidon_mds=True, alpha_chunk=8)
# (inner case, the keywords): `basic` has 30 terms -- chunks of 8 leave a last chunk of 6, chunks of 64 are one chunk
VARIANTS = {"poseidon_route": ("poseidon", ROUTE), "poseidon_chunks": ("poseidon", CHUNKS), "poseidon_both": ("poseidon", BOTH),
            "basic_chunks": ("basic", CHUNKS), "basic_one_chunk": ("basic", dict(alpha_chunk=64))}
_built, _read = {}, {}


def reading(name):
    """the independent reading of the inner case's proof, once"""
    if name not in _read:
        o = cases.inner(name)
        _read[name] = vr.read(cases.oracle_proof(o), cases.INNER_DIGEST, o["c"].log_n, o["circ"], o["params"], cases.CAP_HEIGHT, len(o["pis"]))
    return _read[name]


def build(variant):
    """one variant, once: the inner circuit with the oracle's proof, the vanishing circuit, its arguments"""
    if variant not in _built:
        name, kw = VARIANTS[variant]
        o = cases.inner(name)
        pf = cases.oracle_proof(o)
        c = pv.PlonkVanishingCircuit(o["c"].log_n, o["params"], o["circ"], cases.CAP_HEIGHT, len(o["pis"]), **kw)
        _built[variant] = {"o": o, "proof": pf, "c": c, "cs": c.constants_sigmas(), "args": pv.flat_proof_arguments(c, pf, cases.INNER_DIGEST),
                           "reading": reading(name), "kw": kw}
    return _built[variant]


def witness(b, args=None):
    """(the replayed witness, the public inputs, their hash); the good one of a variant is kept"""
    if args is None:
        if "witness" not in b:
            b["witness"] = witness(b, b["args"])
        return b["witness"]
    c = b["c"]
    pis = c.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    return rd.replay(c.partial_witness(*args), b["cs"][:c.num_constants], c.generators(), pih, c.schedule()), pis, pih


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def whole(request):
    return build(request.param)


# ---- the gate program -------------------------------------------------------------------------------------------------------------------
def _mds_constraints(words, w):
    """the gate's constraint values on one row's wires, in Python integers"""
    circ = {"programs": words, "gates": [(0, 0, 0, 1, 0, 24)]}
    out = []
    for monos in pv.gate_constraints(circ, 0):
        total = 0
        for coef, key in monos:
            for kind, idx in key:
                assert kind == 0
                coef = coef * (w[idx] % P)
            total += coef
        out.append(total % P)
    return out


MDS_LAYOUTS = [(0, 24), (24, 0), (7, 60)]


@pytest.mark.parametrize("in_,out", MDS_LAYOUTS)
def test_the_mds_gate_has_24_linear_constraints_met_by_the_reading_and_each_broken_by_its_output(in_, out):
    words = mk.poseidon_mds_gate(in_, out) if (in_, out) != (0, 24) else mk.poseidon_mds_gate()
    cons = pv.gate_constraints({"programs": words, "gates": [(0, 0, 0, 1, 0, 24)]}, 0)
    assert len(cons) == 24 and all(len(key) == 1 for monos in cons for _, key in monos) and all(len(monos) == 13 for monos in cons)
    assert len(pv.gate_words({"programs": np.concatenate([words, words]), "gates": [(0, 0, 0, 1, 0, 24)]}, 0)) == len(words)
    rng = np.random.default_rng(1601)
    rows = [[0] * 24, [P - 1] * 24, [(1 << 64) - 1] * 24, [P] * 24, [int(v) for v in rng.integers(0, 1 << 64, 24, dtype=np.uint64)],
            [int(v) for v in rng.integers(P, 1 << 64, 24, dtype=np.uint64)]]
    for ins in rows:
        w = [int(v) for v in rng.integers(0, P, 135, dtype=np.uint64)]
        w[in_:in_ + 24] = ins
        pm.mds_row(w, in_, out)
        assert w[in_:in_ + 24] == ins and all(0 <= v < P for v in w[out:out + 24])
        assert _mds_constraints(words, w) == [0] * 24
        for j in range(24):                                     # constraint 2 r + l answers for output cell out + 2 r + l, and no other does
            bad = list(w)
            bad[out + j] = (bad[out + j] + 1) % P
            assert [t for t, v in enumerate(_mds_constraints(words, bad)) if v] == [j]
    # the matrix is the permutation's: a row of the gate against the oracle's linear layer through one full permutation is out of reach,
    # so against sipp_amd.merkle's table, which the swap gate's pinned program is built from
    assert [list(r) for r in mk.poseidon_tables()[1]] == pm.M


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(whole):
    b, c = whole, whole["c"]
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
    assert [at(x) for x in c.alpha_cells] == r["alphas"] and ext(c.zeta_cells) == r["zeta"]
    assert len(c.term_cells) == len(r["terms"]) == c.C + c.C * c.m + c.ngc
    assert [ext(t) for t in c.term_cells] == r["terms"]
    assert [(ext(x), ext(y)) for x, y in c.side_cells] == r["sides"] and all(x == y for x, y in r["sides"])
    # the outputs
    assert ext(c.gzeta_cells) == r["gzeta"] and [at(x) for x in c.state_cells] == r["state"]
    assert pis[c.pi_zeta:] == list(r["zeta"]) + list(r["gzeta"]) + r["state"]


def test_the_variants_are_what_they_are_named_for():
    n_terms = {v: len(build(v)["c"].term_cells) for v in VARIANTS}
    assert n_terms["basic_chunks"] == 30 and 30 % 8 == 6 and n_terms["basic_one_chunk"] <= 64 and n_terms["poseidon_both"] == 145
    for v, (name, kw) in VARIANTS.items():
        c = build(v)["c"]
        assert len(c.mds_rows) == (30 if kw.get("poseidon_mds") else 0)
        assert c.circuit()["gate_names"] == (pv.MDS_GATE_NAMES if kw.get("poseidon_mds") else pv.GATE_NAMES)
        assert all(c.gate[r] == pv.POSEIDON_MDS for r in c.mds_rows) and len(set(c.mds_rows)) == len(c.mds_rows)
        kinds = [g[0] for g in c.generators()]
        assert (pm.GEN_POSEIDON_MDS in kinds) == bool(kw.get("poseidon_mds"))
    # the routed gate set: PoseidonMds in the group of the two extension gates, every filtered constraint at degree 8 or below
    circ = build("poseidon_both")["c"].circuit()
    groups = {name: (lo, hi) for name, (_, _, lo, hi, _, _) in zip(circ["gate_names"], circ["gates"])}
    assert groups["PoseidonMds"] == groups["ArithmeticExt"] == groups["QuotientExt"] == (4, 7) and groups["PoseidonSwap"] == (7, 8)
    for g, (sel, row, lo, hi, _, _) in enumerate(circ["gates"]):
        degree = max((len(key) for monos in pv.gate_constraints(circ, g) for _, key in monos), default=0)
        assert (hi - lo - 1) + (circ["num_selectors"] > 1) + degree <= 8, circ["gate_names"][g]
    mds = circ["gate_names"].index("PoseidonMds")
    assert (pv.gate_words(circ, mds) == mk.poseidon_mds_gate(pv.MDS_IN, pv.MDS_OUT)).all()
    # the defaults build what they built: the same object as without the keywords
    o = cases.inner("basic")
    plain, named = (pv.PlonkVanishingCircuit(o["c"].log_n, o["params"], o["circ"], cases.CAP_HEIGHT, len(o["pis"]), **kw)
                    for kw in ({}, dict(poseidon_mds=False, alpha_chunk=None)))
    assert (plain.constants_sigmas() == named.constants_sigmas()).all() and plain.generators() == named.generators()


# ---- the shape conditions: counted, not measured ------------------------------------------------------------------------------------------
INNER_SHAPES = {"merkle_3_1_1_1": ((3, 1, 1, 1), 120), "merkle_16_9_4_28": ((16, 9, 4, 28), 240)}
_shaped = {}


def shaped(name):
    """the routed circuit with chunks of 8 over inner MerkleOpeningCircuit(*shape), and the monomial route's op counts beside it"""
    if name not in _shaped:
        inner = mk.MerkleOpeningCircuit(*INNER_SHAPES[name][0])
        shape = (inner.log_n, (80, 8, 2), inner.circuit(), cases.CAP_HEIGHT, inner.n_pi)
        _shaped[name] = (pv.PlonkVanishingCircuit(*shape, **BOTH), pv.PlonkVanishingCircuit(*shape), inner)
    return _shaped[name]


def counts(c):
    return {"log_n": c.log_n, "rows_used": c.rows_used, "n_levels": c.n_levels, "mds_rows": len(c.mds_rows), "ops": c.ops.count,
            "gate_ops": [int(x) for x in c.gate_ops]}


@pytest.mark.parametrize("name", sorted(INNER_SHAPES))
def test_the_routed_shape_meets_its_counted_conditions(name):
    c, plain, inner = shaped(name)
    swap = inner.circuit()["gate_names"].index("PoseidonSwap")
    assert c.routed_gates == [swap] and plain.routed_gates == []
    print(name, counts(c), "monomial route:", counts(plain))
    assert c.log_n == 10 and plain.log_n == 13
    assert len(c.mds_rows) <= 30
    assert c.gate_ops[swap] <= 1000 and 6300 <= plain.gate_ops[swap] <= 6500
    assert c.n_levels <= INNER_SHAPES[name][1]
    assert c.gate_ops[:swap] == plain.gate_ops[:swap] and c.gate_monomials == plain.gate_monomials


def synthetic_arguments(c):
    """arguments of the right shape for a circuit without an inner proof at hand (the pinned digests need values, not a valid proof)"""
    caps = [np.arange(4 * c.n_cap, dtype=np.uint64).reshape(c.n_cap, 4) + np.uint64(1000 * (o + 1)) for o in range(3)]
    return ([21, 22, 23, 24], [100 + t for t in range(c.n_pi_inner)], caps, [(7 * k + 1, 11 * k + 2) for k in range(c.n_open)])


def shape_digests(name):
    """{item: sha256} of a pinned routed shape, with its counts: a test variant by its inner proof, an inner shape by synthetic values"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import outer_circuit_shapes as shapes
    if name in VARIANTS:
        c, args = build(name)["c"], build(name)["args"]
    else:
        c = shaped(name)[0]
        args = synthetic_arguments(c)
    return dict(shapes.digests(c, args, args), counts=counts(c))


PINNED = sorted(VARIANTS) + sorted(INNER_SHAPES)


@pytest.mark.parametrize("name", PINNED)
def test_shape_is_the_pinned_one(name):
    want = json.load(open(GOLDEN))[name]
    got = shape_digests(name)
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []


# ---- tampering ----------------------------------------------------------------------------------------------------------------------------
def test_one_tampered_sbox_wire_of_a_partial_round_breaks_only_the_closing_ties():
    b = build("poseidon_both")
    c, o = b["c"], b["o"]
    pf = b["proof"].copy()
    wire = mk.sbox_wire(SWAP_LAYOUT["sbox"], 13, 0)             # the S-box input of partial round 13
    at = 16 + 12 * c.n_cap + 8 + 2 * (c.K + c.R + wire)
    pf[at] = (int(pf[at]) + 1) % P
    assert any(x != y for x, y in vr.read(pf, cases.INNER_DIGEST, o["c"].log_n, o["circ"], o["params"], cases.CAP_HEIGHT, len(o["pis"]))["sides"])
    assert _oracle.plonk_verify_gates(pf, o["cap"], o["op"], o["ofp"], o["circ"], cases.INNER_DIGEST) == -210
    w, pis, pih = witness(b, pv.flat_proof_arguments(c, pf, cases.INNER_DIGEST))
    rows, cycles = satisfied(b, w, pih)
    cell = lambda x: x[0] * c.n + x[1]
    ties = {cell(x) for sides in c.side_cells for side in sides for x in side}
    assert rows == [] and cycles and all(ties & set(cyc) for cyc in cycles)


@pytest.mark.parametrize("which,element,limb", [(0, 0, 0), (14, 5, 1), (29, 11, 0)])
def test_one_tampered_mds_output_cell_breaks_that_rows_constraint(which, element, limb):
    b = build("poseidon_both")
    c = b["c"]
    w, pis, pih = witness(b)
    bad = w.copy()
    r, wire = c.mds_rows[which], pv.MDS_OUT + 2 * element + limb
    bad[wire, r] = np.uint64((int(bad[wire, r]) + 1) % P)
    circ = c.circuit()
    values = _oracle.plonk_gate_constraints_base(circ, bad[:, r], b["cs"][:c.num_constants, r], pih)
    assert [j for j, v in enumerate(values) if v] == [2 * element + limb]
    rows, _ = satisfied(b, bad, pih)
    assert rows == [r]


# ---- the refusals at build ------------------------------------------------------------------------------------------------------------------
def test_refusals_at_build():
    basic, poseidon = cases.inner("basic"), cases.inner("poseidon")
    args = lambda o, **kw: dict(dict(log_n=o["c"].log_n, params=o["params"], circuit=o["circ"], cap_height=4, n_pi_inner=len(o["pis"])), **kw)
    with pytest.raises(AssertionError, match="no inner gate"):
        pv.PlonkVanishingCircuit(**args(basic, poseidon_mds=True))
    # the swap gate with one coefficient changed: the name still says PoseidonSwap, the words do not
    circ = poseidon["circ"]
    swap = circ["gate_names"].index("PoseidonSwap")
    off = circ["gates"][swap][4]
    assert (pv.gate_words(circ, swap) == mk.poseidon_swap_gate()).all()
    words = circ["programs"].copy()
    assert words[off] == 2 and words[off + 1] == 1              # swap^2 - swap: two monomials, the first coefficient 1
    words[off + 1] = 2
    assert pv.circuit_ok(dict(circ, programs=words), 80) is None
    with pytest.raises(AssertionError, match="no inner gate"):
        pv.PlonkVanishingCircuit(**args(poseidon, circuit=dict(circ, programs=words), poseidon_mds=True))
    pv.PlonkVanishingCircuit(**args(poseidon, circuit=dict(circ, programs=words)))      # the monomial route takes any program
    for k in (0, 1, -8, 8.0, True):
        with pytest.raises(AssertionError, match="alpha_chunk"):
            pv.PlonkVanishingCircuit(**args(basic, alpha_chunk=k))


# ---- the pair -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """poseidon under both keywords: both outer proofs by the oracle, and the vanishing proof of the DEFAULT circuit beside them"""
    from tests.test_gpu_fri_generic import to_params
    b = build("poseidon_both")
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
    ffp = fri(f.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    second = _oracle.plonk_prove_gates(fw, fcs, f.log_n, OUTER, ffp, f.circuit(), DIGEST, fpis)
    data = [(_oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap, DIGEST) for cs, c in ((b["cs"], v), (fcs, f))]
    return b, (first, second), data, to_params(ofp), to_params(ffp), to_params(o["ofp"])


def test_the_pair_is_accepted_under_both_keywords_and_a_default_vanishing_proof_is_refused(pair):
    b, (first, second), data, gfp_v, gfp_f, inner_fri = pair
    o = b["o"]
    ver = pv.PlonkProofVerifier(None, o["c"].log_n, o["params"], o["circ"], inner_fri, len(o["pis"]), fri=(gfp_v, gfp_f), verifier_data=data,
                                **BOTH)
    assert ver.vc.poseidon_mds and ver.vc.alpha_chunk == 8 and ver.vc.log_n == 10 and len(ver.vc.mds_rows) == 30
    assert (ver.vc.constants_sigmas() == b["cs"]).all()
    assert ver.verify((first, second), o["cap"], cases.INNER_DIGEST) == o["pis"]
    # the same statement proved through the DEFAULT vanishing circuit: a valid proof of another circuit, of another size
    d = pv.PlonkVanishingCircuit(o["c"].log_n, o["params"], o["circ"], cases.CAP_HEIGHT, len(o["pis"]))
    dcs = d.constants_sigmas()
    dargs = pv.flat_proof_arguments(d, b["proof"], cases.INNER_DIGEST)
    dpis = d.public_inputs(*dargs)
    dpih = _oracle.hash_no_pad(np.array(dpis, dtype=np.uint64))
    dw = rd.replay(d.partial_witness(*dargs), dcs[:d.num_constants], d.generators(), dpih, d.schedule())
    dfp = fri(d.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    other = _oracle.plonk_prove_gates(dw, dcs, d.log_n, OUTER, dfp, d.circuit(), DIGEST, dpis)
    dcap = _oracle.Batch(dcs, d.log_n, rate_bits=3, cap_height=4).cap
    assert _oracle.plonk_verify_gates(other, dcap, OUTER, dfp, d.circuit(), DIGEST) == 0 and dpis == [int(x) for x in first[len(first) - d.n_pi:]]
    with pytest.raises(ValueError, match="vanishing proof"):
        ver.verify((other, second), o["cap"], cases.INNER_DIGEST)
    # and the other way round: the default verifier refuses the routed proof
    from tests.test_gpu_fri_generic import to_params
    plain = pv.PlonkProofVerifier(None, o["c"].log_n, o["params"], o["circ"], inner_fri, len(o["pis"]), fri=(to_params(dfp), gfp_f),
                                  verifier_data=[(dcap, DIGEST), data[1]])
    assert plain.verify((other, second), o["cap"], cases.INNER_DIGEST) == o["pis"]
    with pytest.raises(ValueError, match="vanishing proof"):
        plain.verify((first, second), o["cap"], cases.INNER_DIGEST)
