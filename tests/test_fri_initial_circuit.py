"""FRI's initial combination in the outer circuit on the CPU (sipp_amd/fri_initial.py): the programs of the Reducing, ReducingExtension
and quotient rows against the Python reading of their generators (tests/_fri_initial_reading.py) through oracle/plonk_gates.c; the
circuit of fri_combine_initial over opening proofs made by the oracle's FRI prover, the witness replayed level by level, proved by the
oracle and judged by both verifiers (the oracle's and the library's verify.cpp); every query's `old` is the value the fold circuit
(sipp_amd/fri_fold.py) takes as its first."""
import numpy as np
import pytest

from sipp_amd import fri_fold as ff
from sipp_amd import fri_initial as fi
from tests import _fri_cases as fc
from tests import _fri_fold_reading as fr
from tests import _fri_initial_reading as ir
from tests import _merkle_reading as mr
from tests import _witness_reading as rd
from tests import _oracle, _verify
from tests.test_fri_fold_circuit import CASE_A4, CASE_A16, degree, nonzero, one_gate, rand_row, readers
from tests.test_oracle_plonk import fri

P = _oracle.P
W = 7
DIGEST = (91, 92, 93, 94)


def reducing_edges(rng, K, ext):
    """random rows, then: alpha = 0; alpha = (p - 1, p - 1); old acc and coefficients of p - 1; everything p - 1"""
    rows = [rand_row(rng), rand_row(rng)]
    w = rand_row(rng)
    w[0] = w[1] = 0
    rows.append(w)
    w = rand_row(rng)
    w[0] = w[1] = P - 1
    rows.append(w)
    w = rand_row(rng)
    w[2:4 + (2 if ext else 1) * K] = [P - 1] * (2 + (2 if ext else 1) * K)
    rows.append(w)
    rows.append([P - 1] * 135)
    return rows


@pytest.mark.parametrize("K", [1, 2, 25, 43])
def test_reducing_gate(K):
    """2 K constraints of degree 2, accumulator limb 0 then limb 1; rows filled by the reading satisfy them, the edge rows among them;
    the last accumulator is old alpha^K + sum_i c_i alpha^(K-1-i); a changed accumulator cell fails exactly the constraints that read it"""
    rng = np.random.default_rng(61)
    prog = fi.reducing_gate(K, W)
    lay = fi.reducing_layout(K, False)
    assert lay == {"alpha": 0, "old": 2, "coeffs": 4, "accs": 4 + K, "last": 4 + 3 * K - 2, "num_wires": 4 + 3 * K}
    circ = one_gate(prog, 2 * K)
    cons = mr.decode(prog, 0, 2 * K)
    assert len(cons) == 2 * K and degree(prog, 2 * K) == 2
    for i in range(K):
        assert (1, [(0, 4 + K + 2 * i)]) in cons[2 * i] and (P - 1, [(0, 4 + i)]) in cons[2 * i]
        assert (1, [(0, 5 + K + 2 * i)]) in cons[2 * i + 1] and not any((0, 4 + i) in f for _, f in cons[2 * i + 1])
    rows = reducing_edges(rng, K, False)
    for k, w in enumerate(rows):
        ir.reducing_row(w, K, W)
        assert not nonzero(circ, w), k
    w = rows[0]
    want, al = fr_ext(w[2], w[3]), fr_ext(w[0], w[1])
    for i in range(K):
        want = want * al + w[4 + i]
    assert (w[lay["last"]], w[lay["last"] + 1]) == tuple(want)
    assert rows[2][4 + K:4 + 3 * K] == [v for i in range(K) for v in (rows[2][4 + i], 0)]            # alpha = 0: acc_i = c_i
    for cell in range(4 + K, 4 + 3 * K):
        t = list(rows[1])
        t[cell] = (t[cell] + 1) % P
        bad = nonzero(circ, t)
        assert bad and bad == readers(prog, 2 * K, cell), cell


def fr_ext(a, b):
    from oracle.py import plonky2_generic as g2
    return g2.Ext(a, b)


@pytest.mark.parametrize("K", [1, 2, 19, 32])
def test_reducing_ext_gate(K):
    """the same with extension coefficients: limb 1 of an accumulator takes limb 1 of its coefficient"""
    rng = np.random.default_rng(62)
    prog = fi.reducing_ext_gate(K, W)
    lay = fi.reducing_layout(K, True)
    assert lay == {"alpha": 0, "old": 2, "coeffs": 4, "accs": 4 + 2 * K, "last": 4 + 4 * K - 2, "num_wires": 4 + 4 * K}
    circ = one_gate(prog, 2 * K)
    cons = mr.decode(prog, 0, 2 * K)
    assert len(cons) == 2 * K and degree(prog, 2 * K) == 2
    for i in range(K):
        for l in range(2):
            assert (1, [(0, 4 + 2 * K + 2 * i + l)]) in cons[2 * i + l] and (P - 1, [(0, 4 + 2 * i + l)]) in cons[2 * i + l]
    rows = reducing_edges(rng, K, True)
    for k, w in enumerate(rows):
        ir.reducing_ext_row(w, K, W)
        assert not nonzero(circ, w), k
    w = rows[0]
    want, al = fr_ext(w[2], w[3]), fr_ext(w[0], w[1])
    for i in range(K):
        want = want * al + fr_ext(w[4 + 2 * i], w[5 + 2 * i])
    assert (w[lay["last"]], w[lay["last"] + 1]) == tuple(want)
    assert rows[2][4 + 2 * K:4 + 4 * K] == rows[2][4:4 + 2 * K]                                      # alpha = 0: acc_i = c_i
    for cell in range(4 + 2 * K, 4 + 4 * K):
        t = list(rows[1])
        t[cell] = (t[cell] + 1) % P
        bad = nonzero(circ, t)
        assert bad and bad == readers(prog, 2 * K, cell), cell


@pytest.mark.parametrize("n_ops", [1, 16])
def test_quotient_row(n_ops):
    """the quotient row is an ArithmeticExtension row whose multiplicand the generator fills: out = c0 a m + c1 c holds on rows filled
    by the reading and fails after a change of either limb of m; m times the denominator is the numerator"""
    rng = np.random.default_rng(63)
    prog = ff.arithmetic_ext_gate(n_ops, 1, 2, W)
    circ = one_gate(prog, 2 * n_ops)
    for trial in range(6):
        w = rand_row(rng) if trial < 5 else [P - 1] * 135
        c = [0] + ([int(x) for x in _oracle.rand_field(rng, 2)] if trial % 2 else [1, 0])
        before = list(w)
        ir.quotient_ext_row(w, c[1], c[2], n_ops, W)
        assert [j for j in range(135) if w[j] != before[j]] and all(j % 8 in (2, 3) and j < 8 * n_ops for j in range(135) if w[j] != before[j])
        assert not nonzero(circ, w, c), trial
        k = trial % n_ops
        if c[2] == 0:
            assert tuple(fr_ext(w[8 * k + 2], w[8 * k + 3]) * fr_ext(w[8 * k], w[8 * k + 1])) == (w[8 * k + 6], w[8 * k + 7])
        for l in range(2):
            t = list(w)
            t[8 * k + 2 + l] = (t[8 * k + 2 + l] + 1) % P
            assert nonzero(circ, t, c) == {2 * k, 2 * k + 1} == readers(prog, 2 * n_ops, 8 * k + 2 + l)


@pytest.mark.parametrize("edge", ["denominator_zero", "c0_zero", "zero_norm"])
def test_quotient_row_without_an_inverse_writes_zero(edge):
    """a zero denominator, c0 = 0, and W = 4 with a = (2, 1) (norm 4 - 4 = 0) all write (0, 0); the row's constraints then hold only
    if out = c1 c: the constraints, not the generator, refuse such rows"""
    rng = np.random.default_rng(64)
    Wq = 4 if edge == "zero_norm" else W
    prog = ff.arithmetic_ext_gate(1, 1, 2, Wq)
    circ = one_gate(prog, 2)
    w = rand_row(rng)
    c = [0] + [int(x) for x in _oracle.rand_field(rng, 2)]
    if edge == "denominator_zero":
        w[0] = w[1] = 0
    elif edge == "c0_zero":
        c[1] = 0
    else:
        w[0], w[1] = 2, 1
        assert ir.ext_inv((2 * c[1] % P, c[1]), Wq) == (0, 0)
    ir.quotient_ext_row(w, c[1], c[2], 1, Wq)
    assert (w[2], w[3]) == (0, 0)
    assert nonzero(circ, w, c) == {0, 1}                                     # a random out is not c1 c
    w[6], w[7] = c[2] * w[4] % P, c[2] * w[5] % P
    ir.quotient_ext_row(w, c[1], c[2], 1, Wq)
    assert (w[2], w[3]) == (0, 0) and not nonzero(circ, w, c)
    w[6] = (w[6] + 1) % P
    ir.quotient_ext_row(w, c[1], c[2], 1, Wq)
    assert (w[2], w[3]) == (0, 0) and nonzero(circ, w, c) == {0}


# ---- the circuit ------------------------------------------------------------------------------------------------------------------
def build(case, ks):
    inst = fc.build(case)
    pf = _oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, fc.challenger(case))
    alpha, points, opened, queries, batches, n_columns = ir.initial_data(inst, pf)
    kw = {} if ks is None else {"k_base": ks[0], "k_ext": ks[1]}
    c = fi.FriInitialCircuit(inst.log_n + inst.fp.rate_bits, n_columns, batches, len(queries), **kw)
    cs = c.constants_sigmas()
    cs_cap = _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap
    return {"inst": inst, "proof": pf, "args": (alpha, points, opened, queries), "batches": batches, "c": c, "cs": cs, "cs_cap": cs_cap}


@pytest.fixture(scope="module", params=[(CASE_A16, (2, 2)), (CASE_A16, None), (CASE_A4, (2, 2)), (CASE_A4, None)],
                ids=lambda p: "%r-%s" % (p[0], "k2" if p[1] else "kmax"))
def initial(request):
    return build(*request.param)


@pytest.fixture(scope="module")
def initial16():
    return build(CASE_A16, (2, 2))


def witness(o, args=None):
    c = o["c"]
    args = o["args"] if args is None else args
    pis = c.public_inputs(*args)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(c.partial_witness(*args), o["cs"][:5], c.generators(), pih, c.schedule())
    return w, pis, pih


def prove_and_judge(o, w, pis):
    c = o["c"]
    op = _oracle.plonk_params(80, 8, 2)
    ofp = fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    circ = c.circuit()
    pf = _oracle.plonk_prove_gates(w, o["cs"], c.log_n, op, ofp, circ, DIGEST, pis)
    return _oracle.plonk_verify_gates(pf, o["cs_cap"], op, ofp, circ, DIGEST), _verify.lib_plonk_verify(pf, o["cs_cap"], op, ofp, circ, DIGEST)


def test_initial_circuit_shape(initial):
    """five columns: the zeta batch takes all of them, the g zeta batch three; with K = 2 the chains of five are three rows whose first
    carries one coefficient behind a zero; the defaults are the largest K with routed coefficient and last-accumulator cells; degrees
    within 8, every cell on at most one cycle, cycles below the routed wires, at most 16 generators"""
    c = initial["c"]
    circ = c.circuit()
    assert (c.log_m, c.n_columns, c.batches, c.n_queries) == (11, 5, [[0, 1, 2, 3, 4], [1, 3, 4]], 4)
    assert circ["num_wires"] == 135 and circ["num_routed"] == 80 and len(c.generators()) <= 16
    assert [g[1] for g in circ["gates"]] == list(range(10))
    assert [g[5] for g in circ["gates"]] == [0, 4, 1, 1 + c.log_m, 2, 2 * c.k_base, 2 * c.k_ext, 2, c.log_m + 1, 123]
    for (si, row, lo, hi, off, nc), d in zip(circ["gates"], [0, 1, 1, 2, 3, 2, 2, 3, 4, 7]):
        cons = mr.decode(circ["programs"], off, nc)
        assert max([len(f) for cn in cons for _, f in cn] or [0]) == d
        assert (hi - lo - 1) + 1 + d <= 8 and lo <= row < hi
    if (c.k_base, c.k_ext) == (2, 2):
        assert [len(r) for r in c.opened_row] == [3, 2] and [len(r) for r in c.leaf_row[0]] == [3, 2]
        n = c.n
        zero = 0 * n + c.zero_row
        first = c.leaf_row[1][0][0]
        cyc = next(cy for cy in c.cycles if zero in cy)
        assert 4 * n + first in cyc and 5 * n + first not in cyc              # one leading zero coefficient, then column 4
        first = c.opened_row[0][0]
        assert 4 * n + first in cyc and 5 * n + first in cyc and 6 * n + first not in cyc
    else:
        assert (c.k_base, c.k_ext) == (25, 19)
        assert 3 * c.k_base + 4 <= 80 < 3 * (c.k_base + 1) + 4 and 4 * c.k_ext + 4 <= 80 < 4 * (c.k_ext + 1) + 4
        assert [len(r) for r in c.opened_row] == [1, 1]
    assert [len(r) for r in c.power_row] == [3, 2]                            # alpha^5: square, square, multiply; alpha^3: square, multiply
    assert max(max(cy) for cy in c.cycles) < 80 * c.n
    cells = [x for cy in c.cycles for x in cy]
    assert len(cells) == len(set(cells))
    with pytest.raises(AssertionError):
        fi.FriInitialCircuit(11, 5, [[0, 1], []], 4)


def test_initial_circuit_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(initial):
    o, c = initial, initial["c"]
    w, pis, pih = witness(o)
    circ = c.circuit()
    for r in range(c.n):
        assert not _oracle.plonk_gate_constraints_base(circ, w[:, r], o["cs"][:5, r], pih).any(), (r, fi.GATE_NAMES[int(c.gate[r])])
    flat = w.reshape(-1)
    for cyc in c.cycles:
        assert len(set(flat[np.asarray(cyc, dtype=np.int64)].tolist())) == 1
    assert (w[12:16, c.chain_row[-1]] == pih).all()
    # the link to FriFoldCircuit: every query's old is the first old of the fold data of the same proof
    _, _, fold_queries = fr.fold_data(o["inst"], o["proof"])
    for q, ((x, leaves, old), (fx, fold_old, _)) in enumerate(zip(o["args"][3], fold_queries)):
        assert x == fx and old == fold_old
        assert (int(w[6, c.old_row[q]]), int(w[7, c.old_row[q]])) == old
    assert prove_and_judge(o, w, pis) == (0, 0)


@pytest.mark.parametrize("tamper", ["leaf_value", "opened_value", "point", "old"])
def test_tampered_inputs_give_proofs_both_verifiers_refuse(initial16, tamper):
    o = initial16
    alpha, points, opened, queries = o["args"]
    points, opened, queries = list(points), [list(v) for v in opened], [(x, list(lv), old) for x, lv, old in queries]
    bump = lambda p, l: tuple((v + (k == l)) % P for k, v in enumerate(p))
    if tamper == "leaf_value":
        queries[1][1][3] = (queries[1][1][3] + 1) % P
    elif tamper == "opened_value":
        opened[1][2] = bump(opened[1][2], 1)
    elif tamper == "point":
        points[0] = bump(points[0], 0)
    else:
        queries[2] = (queries[2][0], queries[2][1], bump(queries[2][2], 1))
    w, pis, _ = witness(o, (alpha, points, opened, queries))
    orc, lib = prove_and_judge(o, w, pis)
    assert orc != 0 and lib != 0, (orc, lib)
