"""FRI fold chains in the outer circuit on the CPU (sipp_amd/fri_fold.py): the programs of the ArithmeticExtension, Exponentiation and
CosetInterpolation gates against the Python reading of their rows (tests/_fri_fold_reading.py) through oracle/plonk_gates.c; the
fold-checking circuit over opening proofs made by the oracle's FRI prover, the witness replayed level by level, proved by the oracle and
judged by both verifiers (the oracle's and the library's verify.cpp)."""
import numpy as np
import pytest

from oracle.py import plonky2_generic as g2
from sipp_amd import fri_fold as ff
from tests import _fri_cases as fc
from tests import _fri_fold_reading as fr
from tests import _merkle_reading as mr
from tests import _witness_reading as rd
from tests import _oracle, _verify
from tests.test_oracle_plonk import fri

P = _oracle.P
W = 7
DIGEST = (71, 72, 73, 74)
INTERP_SHAPES = [(1, 2), (1, 7), (2, 2), (2, 3), (2, 7), (3, 2), (3, 4), (3, 7), (4, 2), (4, 4), (4, 6), (4, 7), (4, 16)]
CASE_A16 = fc.Case("fold-arity16", log_n=10, rate_bits=1, cap_height=2, widths=(3, 2), seed=31,
                   fri=dict(arity_bits=4, final_poly_bits=2, num_queries=4))
CASE_A4 = fc.Case("fold-arity4", log_n=10, rate_bits=1, cap_height=2, widths=(3, 2), seed=32,
                  fri=dict(arity_bits=2, final_poly_bits=4, num_queries=4))


def one_gate(prog, count, num_wires=135, num_constants=3):
    return {"num_wires": num_wires, "num_routed": 80, "num_constants": num_constants, "num_selectors": 1, "gates": [(0, 0, 0, 1, 0, count)],
            "programs": prog, "num_gate_constraints": count}


def nonzero(circ, w, consts=(0, 0, 0)):
    return set(np.flatnonzero(_oracle.plonk_gate_constraints_base(circ, np.array(w, dtype=np.uint64), np.array(consts, dtype=np.uint64),
                                                                  [0, 0, 0, 0])).tolist())


def readers(prog, count, wire):
    """the constraints whose program reads the wire"""
    return {j for j, c in enumerate(mr.decode(prog, 0, count)) if any((0, wire) in f for _, f in c)}


def degree(prog, count):
    return max(len(f) for c in mr.decode(prog, 0, count) for _, f in c)


def rand_row(rng, num_wires=135):
    return [int(x) for x in _oracle.rand_field(rng, num_wires)]


# ---- the three gate programs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ops", [1, 16])
def test_arithmetic_ext_gate(n_ops):
    """2 constraints per op, output limb 0 then limb 1, degree 3 (constant column, two wires); random rows and rows of p - 1 satisfy it;
    a tampered output limb fails its own constraint alone"""
    rng = np.random.default_rng(41)
    prog = ff.arithmetic_ext_gate(n_ops, 1, 2, W)
    circ = one_gate(prog, 2 * n_ops)
    cons = mr.decode(prog, 0, 2 * n_ops)
    assert len(cons) == 2 * n_ops and degree(prog, 2 * n_ops) == 3
    for k in range(n_ops):
        for l in range(2):
            assert (1, [(0, 8 * k + 6 + l)]) in cons[2 * k + l]              # output - computed
            assert (P - 1, [(0, 8 * k + 4 + l), (1, 2)]) in cons[2 * k + l]             # factors sorted: (wire, index) before (constant, index)
    for trial in range(8):
        w = rand_row(rng) if trial < 6 else [P - 1] * 135
        c = [0] + ([int(x) for x in _oracle.rand_field(rng, 2)] if trial % 2 else [P - 1, P - 1])
        fr.arithmetic_ext_row(w, c[1], c[2], n_ops, W)
        assert not nonzero(circ, w, c), trial
        k = trial % n_ops
        for l in range(2):
            t = list(w)
            t[8 * k + 6 + l] = (t[8 * k + 6 + l] + 1) % P
            assert nonzero(circ, t, c) == {2 * k + l} == readers(prog, 2 * n_ops, 8 * k + 6 + l)


@pytest.mark.parametrize("n_bits", [1, 11, 64])
def test_exponentiation_gate(n_bits):
    """n_bits constraints  prev^2 (bit base + 1 - bit) - intermediate_i  (bits from the top wire down), then output - last intermediate;
    degree 4 (2 when there is one bit); with 0 / 1 bits the output is base^exponent; base 0 and p - 1; a bit of 2 gives the generator's
    defined values and satisfies the gate (upstream's gate has no booleanity constraint)"""
    rng = np.random.default_rng(42)
    prog = ff.exponentiation_gate(n_bits)
    circ = one_gate(prog, n_bits + 1)
    cons = mr.decode(prog, 0, n_bits + 1)
    assert len(cons) == n_bits + 1 and degree(prog, n_bits + 1) == (4 if n_bits > 1 else 2)
    for i in range(n_bits):
        assert (P - 1, [(0, 2 + n_bits + i)]) in cons[i]
        assert any(sorted(f) == sorted([(0, 1 + n_bits + i)] * 2 * (i > 0) + [(0, n_bits - i), (0, 0)]) for _, f in cons[i])
    norm = lambda c: sorted((k, tuple(sorted(f))) for k, f in c)
    assert norm(cons[n_bits]) == norm([(1, [(0, 1 + n_bits)]), (P - 1, [(0, 1 + 2 * n_bits)])])
    for base in (None, 0, P - 1, None):
        w = rand_row(rng)
        if base is not None:
            w[0] = base
        e = int(rng.integers(0, 1 << 63)) % (1 << n_bits) | (1 << (n_bits - 1))
        for j in range(n_bits):
            w[1 + j] = (e >> j) & 1
        fr.exponentiation_row(w, n_bits)
        assert w[1 + n_bits] == pow(w[0], e, P)
        assert not nonzero(circ, w)
        i = n_bits // 2
        t = list(w)
        t[2 + n_bits + i] = (t[2 + n_bits + i] + 1) % P
        assert nonzero(circ, t) == readers(prog, n_bits + 1, 2 + n_bits + i) == ({i, i + 1} if i + 1 < n_bits else {i, n_bits})
        t = list(w)
        t[1 + n_bits] = (t[1 + n_bits] + 1) % P
        assert nonzero(circ, t) == {n_bits}
    w = rand_row(rng)                                                        # any field value in a bit wire
    w[1:1 + n_bits] = [2] + [int(x) for x in rng.integers(0, 2, size=n_bits - 1)]
    fr.exponentiation_row(w, n_bits)
    last = w[1 + 2 * n_bits - 1] if n_bits > 1 else 1
    assert w[1 + n_bits] == last * last * (2 * w[0] + 1 - 2) % P
    assert not nonzero(circ, w)


def interp_row(rng, s, d, shift=None, point=None, values=None):
    w = rand_row(rng)
    n = 1 << s
    if shift is not None:
        w[0] = shift
    if point is not None:
        w[1 + 2 * n], w[2 + 2 * n] = point
    if values is not None:
        w[1:1 + 2 * n] = [values] * (2 * n)
    fr.coset_interpolation_row(w, s, d, W)
    return w


@pytest.mark.parametrize("s,d", INTERP_SHAPES)
def test_coset_interpolation_gate(s, d):
    """2 (shifted shift - point) + 4 per intermediate (eval limbs, product limbs) + 2 (the evaluation value) constraints of degree
    min(d, n); rows filled by the reading satisfy them, also with shift = point = 0, a point on the coset (a zero term) and values of
    p - 1; the value is the interpolant's (compute_evaluation's barycentric form with the weights' identity g^i / n)"""
    rng = np.random.default_rng(43)
    n = 1 << s
    lay = ff.interpolation_layout(s, d)
    ni = (n - 2) // (d - 1)
    count = 4 + 4 * ni
    assert lay["ni"] == ni and lay["num_wires"] == 1 + 2 * n + 4 + 4 * ni + 2
    prog = ff.coset_interpolation_gate(s, d, W)
    circ = one_gate(prog, count)
    cons = mr.decode(prog, 0, count)
    assert len(cons) == count and degree(prog, count) == min(d, n)
    assert max(len(c) for c in cons) <= ff.MAX_MONOMIALS
    sh, start = lay["shifted"], 5 + 2 * n
    norm = lambda c: sorted((k, tuple(sorted(f))) for k, f in c)
    for l in range(2):
        assert norm(cons[l]) == norm([(1, [(0, sh + l), (0, 0)]), (P - 1, [(0, 1 + 2 * n + l)])])
        assert (P - 1, [(0, 3 + 2 * n + l)]) in cons[count - 2 + l]
    for c in range(ni):
        for l in range(2):
            assert (P - 1, [(0, start + 2 * c + l)]) in cons[2 + 4 * c + l]                      # computed eval - wire
            assert (P - 1, [(0, start + 2 * ni + 2 * c + l)]) in cons[2 + 4 * c + 2 + l]         # computed product - wire
    xs, ws = fr.domain(s)
    g = g2.primitive_root_of_unity(s)
    assert xs == [pow(g, i, P) for i in range(n)] and ws == [x * pow(n, P - 2, P) % P for x in xs]
    x3 = xs[min(3, n - 1)]
    rows = [interp_row(rng, s, d), interp_row(rng, s, d), interp_row(rng, s, d, shift=0, point=(0, 0)),
            interp_row(rng, s, d, shift=5, point=(5 * x3 % P, 0)), interp_row(rng, s, d, shift=P - 1, point=(P - 1, P - 1), values=P - 1)]
    for k, w in enumerate(rows):
        assert not nonzero(circ, w), k
    # the value: sum_i value_i prod_(k != i) (z - x_k) / prod_(k != i) (x_i - x_k) at z = point / shift
    w = rows[0]
    z = g2.Ext(w[1 + 2 * n], w[2 + 2 * n]) * g2.inv(w[0])
    total = g2.Ext(0)
    for i in range(n):
        num, den = g2.Ext(w[1 + 2 * i], w[2 + 2 * i]), 1
        for k in range(n):
            if k != i:
                num, den = num * (z - xs[k]), den * (xs[i] - xs[k]) % P
        total = total + num * g2.inv(den)
    assert (w[3 + 2 * n], w[4 + 2 * n]) == tuple(total)
    assert (rows[2][sh], rows[2][sh + 1]) == (0, 0) and (rows[3][sh], rows[3][sh + 1]) == (x3, 0)
    # a tampered written cell fails exactly the constraints that read it
    for cell in sorted({sh, sh + 1, 3 + 2 * n, 4 + 2 * n} | set(range(start, start + 4 * ni))):
        t = list(rows[1])
        t[cell] = (t[cell] + 1) % P
        assert nonzero(circ, t) == readers(prog, count, cell), cell


def test_interpolation_equals_compute_evaluation():
    """values = the bit-reversed evals, shift = x (g^-1)^rev(index within the coset): the row's value is fri/verifier.rs
    compute_evaluation, s = 1 .. 4"""
    rng = np.random.default_rng(44)
    for s, d in INTERP_SHAPES:
        n = 1 << s
        evals = [g2.Ext(*[int(v) for v in _oracle.rand_field(rng, 2)]) for _ in range(n)]
        beta = g2.Ext(*[int(v) for v in _oracle.rand_field(rng, 2)])
        x, within = int(_oracle.rand_field(rng, 1)[0]), int(rng.integers(0, n))
        w = [0] * 135
        w[0] = x * pow(g2.inv(g2.primitive_root_of_unity(s)), g2.reverse_bits(within, s), P) % P
        for k in range(n):
            w[1 + 2 * k], w[2 + 2 * k] = evals[g2.reverse_bits(k, s)]
        w[1 + 2 * n], w[2 + 2 * n] = beta
        fr.coset_interpolation_row(w, s, d, W)
        assert (w[3 + 2 * n], w[4 + 2 * n]) == tuple(g2.compute_evaluation(x, within, s, evals, beta)), (s, d)


# ---- the fold-checking circuit -------------------------------------------------------------------------------------------------------------
def build(case, seed_shift=0):
    inst = fc.build(case)
    pf = _oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, fc.challenger(case))
    betas, final_poly, queries = fr.fold_data(inst, pf)
    fp = inst.fp
    arities = [fp.arity_bits[i] for i in range(fp.n_rounds)]
    assert len(set(arities)) == 1
    c = ff.FriFoldCircuit(inst.log_n + fp.rate_bits, arities[0], len(arities), len(final_poly), len(queries))
    cs = c.constants_sigmas()
    cs_cap = _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap
    return {"inst": inst, "betas": betas, "final": final_poly, "queries": queries, "c": c, "cs": cs, "cs_cap": cs_cap}


@pytest.fixture(scope="module", params=[CASE_A16, CASE_A4], ids=repr)
def folds(request):
    return build(request.param)


@pytest.fixture(scope="module")
def folds16():
    return build(CASE_A16)


def witness(o, betas=None, final=None, queries=None):
    c = o["c"]
    args = (o["betas"] if betas is None else betas, o["final"] if final is None else final, o["queries"] if queries is None else queries)
    pis = c.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(c.partial_witness(*args), o["cs"][:6], c.generators(), pih, c.schedule())
    return w, pis, pih


def prove_and_judge(o, w, pis):
    c = o["c"]
    op = _oracle.plonk_params(80, 8, 2)
    ofp = fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    circ = c.circuit()
    pf = _oracle.plonk_prove_gates(w, o["cs"], c.log_n, op, ofp, circ, DIGEST, pis)
    return _oracle.plonk_verify_gates(pf, o["cs_cap"], op, ofp, circ, DIGEST), _verify.lib_plonk_verify(pf, o["cs_cap"], op, ofp, circ, DIGEST)


def test_fold_cases_have_the_stated_shape(folds):
    inst, c = folds["inst"], folds["c"]
    if inst.case is CASE_A16:
        assert (c.arity_bits, c.n_rounds, c.final_len, c.n_queries, c.log_m) == (4, 2, 4, 4, 11)
    else:
        assert (c.arity_bits, c.n_rounds, c.final_len, c.n_queries, c.log_m) == (2, 3, 16, 4, 11)


def test_fold_circuit_shape(folds):
    """degrees within 8, every cell on at most one cycle, cycles below the routed wires, at most 16 generators"""
    c = folds["c"]
    circ = c.circuit()
    assert circ["num_wires"] == 135 and circ["num_routed"] == 80 and len(c.generators()) <= 16
    assert [g[1] for g in circ["gates"]] == list(range(9))
    lay = ff.interpolation_layout(c.arity_bits, ff.INTERP_DEGREE)
    assert [g[5] for g in circ["gates"]] == [0, 4, 1, 1 + c.log_m, 2, 2 * (c.arity_bits + 2), c.log_m + 1, 123, 4 + 4 * lay["ni"]]
    for (si, row, lo, hi, off, nc), d in zip(circ["gates"], [0, 1, 1, 2, 3, c.arity_bits + 1, 4, 7, min(7, c.arity)]):
        cons = mr.decode(circ["programs"], off, nc)
        assert max([len(f) for cn in cons for _, f in cn] or [0]) == d
        assert max([len(cn) for cn in cons] or [0]) <= 4096
        assert (hi - lo - 1) + 1 + d <= 8
        assert lo <= row < hi
    assert ff.INTERP_DEGREE == 7                                             # alone in its group: the largest the filter leaves room for
    assert max(max(cy) for cy in c.cycles) < 80 * c.n
    cells = [x for cy in c.cycles for x in cy]
    assert len(cells) == len(set(cells))


def test_fold_circuit_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(folds):
    o, c = folds, folds["c"]
    w, pis, pih = witness(o)
    circ = c.circuit()
    for r in range(c.n):
        assert not _oracle.plonk_gate_constraints_base(circ, w[:, r], o["cs"][:6, r], pih).any(), (r, ff.GATE_NAMES[int(c.gate[r])])
    flat = w.reshape(-1)
    for cyc in c.cycles:
        assert len(set(flat[np.asarray(cyc, dtype=np.int64)].tolist())) == 1
    assert (w[12:16, c.chain_row[-1]] == pih).all()
    # the interpolation rows' values are compute_evaluation's, the x of every round is the verifier's
    ev = c.interp["eval"]
    for q, (x_index, old, evals) in enumerate(o["queries"]):
        x = g2.GEN * pow(g2.primitive_root_of_unity(c.log_m), g2.reverse_bits(x_index, c.log_m), P) % P
        assert int(w[6, c.x_row[q]]) == x
        for r in range(c.n_rounds):
            within = (x_index >> (c.arity_bits * r)) & (c.arity - 1)
            want = g2.compute_evaluation(x, within, c.arity_bits, [g2.Ext(*v) for v in evals[r]], g2.Ext(*o["betas"][r]))
            row = c.interp_row[q][r]
            assert (int(w[ev, row]), int(w[ev + 1, row])) == tuple(want), (q, r)
            x = pow(x, c.arity, P)
            assert int(w[6, c.sq_row[q][r][-1]]) == x
    assert prove_and_judge(o, w, pis) == (0, 0)


def _bump(pair, l=0):
    p = list(pair)
    p[l] = (p[l] + 1) % P
    return tuple(p)


@pytest.mark.parametrize("tamper", ["eval_at_within", "eval_elsewhere", "beta_limb", "final_coefficient", "x_index_bit", "first_old"])
def test_tampered_folds_give_proofs_both_verifiers_refuse(folds16, tamper):
    o, c = folds16, folds16["c"]
    betas, final, queries = list(o["betas"]), list(o["final"]), [(x, old, [list(r) for r in ev]) for x, old, ev in o["queries"]]
    x_index, old, ev = queries[1]
    within1 = (x_index >> c.arity_bits) & (c.arity - 1)
    if tamper == "eval_at_within":
        ev[1][within1] = _bump(ev[1][within1], 1)
    elif tamper == "eval_elsewhere":
        ev[1][within1 ^ 5] = _bump(ev[1][within1 ^ 5])
    elif tamper == "beta_limb":
        betas[0] = _bump(betas[0], 1)
    elif tamper == "final_coefficient":
        final[2] = _bump(final[2])
    elif tamper == "x_index_bit":
        queries[1] = (x_index ^ (1 << 6), old, ev)
    else:
        queries[1] = (x_index, _bump(old), ev)
    w, pis, _ = witness(o, betas, final, queries)
    orc, lib = prove_and_judge(o, w, pis)
    assert orc != 0 and lib != 0, (orc, lib)
