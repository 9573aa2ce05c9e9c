"""The permutation-argument catalogue of tests/_perm_cases.py on the CPU: oracle/plonk.c cell for cell against the catalogue's
Python-integer expectation, the closed forms against both, the second reading (oracle/py/plonky2_generic.py) on the small entries, proof
that every edge class the catalogue claims is really reached, and the section-B configurations through the oracle's prove / verify pair."""
import numpy as np
import pytest

from tests import _oracle
from tests import _perm_cases as pc

P = pc.P
A = dict(pc.ENTRIES_A)
B = dict(pc.ENTRIES_B)


def oracle_zs(e):
    wires, sigmas, betas, gammas = pc.oracle_inputs(e)
    return _oracle.plonk_zs(wires, sigmas, e["log_n"], _oracle.plonk_params(e["R"], e["D"], e["C"]), betas, gammas)


@pytest.mark.parametrize("name", pc.IDS_A)
def test_oracle_matches_the_integer_reference(name):
    """oracle/plonk.c (given canonical operands) against zs_exact, every cell; the closed form, where the entry names one, on both"""
    e = A[name]()
    got = oracle_zs(e)
    assert got.shape == e["zs"].shape == (e["C"] * pc.num_chunks(e["R"], e["D"]), 1 << e["log_n"])
    msg = pc.first_mismatch(got, e["zs"])
    assert msg is None, msg
    if e["closed"]:
        form = pc.CLOSED_FORMS[e["closed"]]
        assert form(e), e["closed"]
        assert form(dict(e, zs=got)), "oracle: " + e["closed"]
    if e["reduced"]:          # some operand really is non-canonical, and the expectation is that of the reduced operands
        raw = [int(v) for v in e["wires"].reshape(-1)] + e["betas"] + e["gammas"]
        assert any(v >= P for v in raw)
        w, s, b, g = pc.oracle_inputs(e)
        assert (pc.zs_exact(w, s, e["log_n"], e["D"], b, g)[0] == e["zs"]).all()


@pytest.mark.parametrize("name", [n for n in pc.IDS_A if "_n9_" not in n and "n12" not in n and "n10" not in n])
def test_second_reading_agrees_on_the_small_entries(name):
    """oracle/py/plonky2_generic.py::wires_permutation_partial_products_and_zs (one inversion per WIRE, 1 / 0 = 0) on every entry with
    N <= 2^5: its columns are the partial products, then Z"""
    from oracle.py import plonky2_generic as g
    e = A[name]()
    assert e["log_n"] <= 5
    wires, sigmas, betas, gammas = pc.oracle_inputs(e)
    w, s = [[int(v) for v in r] for r in wires], [[int(v) for v in r] for r in sigmas]
    C, npp = e["C"], pc.num_chunks(e["R"], e["D"]) - 1
    for c in range(C):
        cols = g.wires_permutation_partial_products_and_zs(w, s, betas[c], gammas[c], e["D"])
        assert len(cols) == npp + 1
        assert cols[-1] == [int(v) for v in e["zs"][c]], "Z of challenge %d" % c
        for q in range(npp):
            assert cols[q] == [int(v) for v in e["zs"][C + c * npp + q]], "partial product %d of challenge %d" % (q, c)


def _den(e, c, j, i):
    return (int(e["wires"][j, i]) + e["betas"][c] * int(e["sigmas"][j, i]) + e["gammas"][c]) % P


def _num(e, c, j, i):
    x = pow(pc.root_of_unity(e["log_n"]), i, P)
    return (int(e["wires"][j, i]) + e["betas"][c] * pc.k_i(j) * x + e["gammas"][c]) % P


def _cols(e, c):
    """Z and the partial products of challenge c, in chunk order"""
    npp = pc.num_chunks(e["R"], e["D"]) - 1
    return [e["zs"][c]] + [e["zs"][e["C"] + c * npp + q] for q in range(npp)]


def test_the_catalogue_reaches_its_edges():
    """every class of the issue has an entry that really has it: computed from the entries' data, not read off their names"""
    entries = [f() for _, f in pc.ENTRIES_A]
    by_class = {}
    for e in entries:
        for k in e["classes"]:
            by_class.setdefault(k, []).append(e)
    chunks = lambda e: pc.num_chunks(e["R"], e["D"])
    # shapes
    for log_n in pc.SHAPE_LOG_NS:
        got = {(e["R"], e["D"], e["C"]) for e in by_class["log_n_%d" % log_n] if e["name"].startswith("shape")}
        assert got == {(R, D, C) for R, D, C, _ in pc.SHAPES}, log_n
    assert set(pc.SHAPE_LOG_NS) == {1, 5, 9, 12}
    assert all(chunks(e) == 1 for e in by_class["one_chunk"]) and {(e["R"], e["D"]) for e in by_class["one_chunk"]} == {(1, 2), (8, 8)}
    assert all(chunks(e) == pc.MAX_CHUNKS == 32 for e in by_class["chunks_32"]) and {e["R"] for e in by_class["chunks_32"]} == {63, 64}
    assert all(e["C"] == pc.MAX_CHALLENGES == 8 for e in by_class["challenges_8"])
    assert all(e["R"] % e["D"] == 1 and chunks(e) > 1 for e in by_class["ragged_one_wire"]) and any(e["R"] == 9 for e in by_class["ragged_one_wire"])
    assert all(16 <= e["D"] <= 64 for e in by_class["chunk_size_16_to_64"]) and any(e["D"] == 64 and e["R"] == 65 for e in by_class["chunk_size_16_to_64"])
    # the refusals sit one step outside check()'s limits
    ref = {name: (log_n, R, D, C, code) for name, log_n, R, D, C, code in pc.REFUSALS_A}
    assert pc.num_chunks(*ref["chunks_33"][1:3]) == 33 and ref["challenges_9"][3] == 9 and ref["log_n_0"][0] == 0 and ref["log_n_25"][0] == 25
    assert [ref[k][2] for k in ("chunk_size_3", "chunk_size_1", "chunk_size_128")] == [3, 1, 128]
    assert all(ref[k][4] == pc.E_UNSUPPORTED for k in ref if not k.startswith("log_n")) and ref["log_n_0"][4] == ref["log_n_25"][4] == pc.E_BADARG
    # closed forms
    assert {e["closed"] for e in by_class["closed_form"]} == set(pc.CLOSED_FORMS)
    ident = A["identity"]()
    assert (ident["sigmas"] == pc.identity_sigmas(ident["log_n"], ident["R"])).all() and all(b % P for b in ident["betas"])
    assert all(b == 0 for b in A["beta_zero"]()["betas"]) and not (A["beta_zero"]()["sigmas"] == pc.identity_sigmas(5, 13)).all()
    assert sorted(int(A["constant_wires_%d" % k]()["wires"][0, 0]) for k in range(6)) == sorted(pc.EDGE_VALUES)
    assert all(len(set(A["constant_wires_%d" % k]()["wires"].reshape(-1).tolist())) == 1 for k in range(6))
    (ja, ia), (jb, ib) = pc.TRANSPOSITION
    tr = A["transposition"]()
    assert ja // tr["D"] != jb // tr["D"] and ja != jb and ia != ib
    ids = pc.identity_sigmas(tr["log_n"], tr["R"])
    assert tr["sigmas"][ja, ia] == ids[jb, ib] and tr["sigmas"][jb, ib] == ids[ja, ia] and (tr["sigmas"] != ids).sum() == 2
    # vanishing denominators: 0 mod p at the stated cells, in the stated chunks; that chunk's partial product is the first 0 of its row
    want_chunks = {"den_chunk_0": [0], "den_chunk_2": [2], "den_ragged_last": [3], "den_two_chunks": [1, 2], "den_zero_over_zero": [1],
                   "den_chunk_2_n12": [2]}
    for name, qs in want_chunks.items():
        e = A[name]()
        assert e["C"] == 3 and [j // e["D"] for _, j, _ in e["cells"]] == qs
        for c, j, i in e["cells"]:
            assert c == pc.SPECIAL and _den(e, c, j, i) == 0
            assert (_num(e, c, j, i) == 0) == (name == "den_zero_over_zero")
        row = e["cells"][0][2]
        cols = _cols(e, pc.SPECIAL)
        assert all(int(cols[q][row]) != 0 for q in range(qs[0] + 1)), "the products before the vanishing chunk stay non-zero"
        assert all(int(cols[q][row]) == 0 for q in range(qs[0] + 1, len(cols)))
        assert (cols[0][row + 1:] == 0).all() and (cols[0][:row + 1] != 0).all()
        others = [c for c in range(3) if c != pc.SPECIAL]
        assert all((col != 0).all() for c in others for col in _cols(e, c)), "the other challenges' columns never see the zero"
    assert A["den_ragged_last"]()["cells"][0][1] == 12 and 13 % 4 == 1
    assert any(e["log_n"] == 12 for e in by_class["vanishing_denominator"])
    # vanishing numerators: Z is 0 from the next row on (never, for the last row)
    want_rows = {"num_row_0": (5, [0]), "num_row_last": (5, [31]), "num_rows_3_4_n12": (12, [3, 4]), "num_row_3_n12": (12, [3]),
                 "num_row_4_n12": (12, [4]), "num_row_1023_n10": (10, [1023])}
    for name, (log_n, rows) in want_rows.items():
        e = A[name]()
        assert e["log_n"] == log_n and [i for _, _, i in e["cells"]] == rows
        for c, j, i in e["cells"]:
            assert c == 0 and _num(e, c, j, i) == 0 and _den(e, c, j, i) != 0
        z = e["zs"][0]
        assert (z[:rows[0] + 1] != 0).all() and (z[rows[0] + 1:] == 0).all()
        q = e["cells"][0][1] // e["D"]
        assert all(int(col[rows[0]]) == 0 for col in _cols(e, 0)[q + 1:]), "the row's own partial products from the chunk on"
        assert (e["zs"][1] != 0).all()
    assert (1 << 12) // 1024 == 4, "rows 3 and 4 of log_n 12 belong to scan threads 0 and 1"
    # operand edges
    assert set(A["edge_wires"]()["wires"].reshape(-1).tolist()) == set(pc.EDGE_VALUES)
    ec = A["edge_challenges"]()
    assert set(ec["betas"]) == set(ec["gammas"]) == {0, 1, P - 1, P, P + 1, 2**64 - 1} and ec["reduced"]
    nw = A["noncanonical_wires"]()["wires"]
    assert (nw >= np.uint64(P)).sum() > nw.size // 4 and int(nw.max()) == 2**64 - 1 and int(nw[0, 0]) == P
    # section B
    eb = [f() for _, f in pc.ENTRIES_B]
    cfg = {(e["log_n"], e["R"], e["D"], e["C"], e["rate_bits"]) for e in eb if e["kind"] == "proof"}
    assert {(10, 9, 2, 1, 3), (10, 13, 4, 2, 3), (10, 9, 2, 1, 2), (10, 63, 2, 1, 1), (10, 5, 2, 8, 1), (10, 1, 2, 1, 1), (10, 8, 8, 2, 3)} <= cfg
    assert any(e["log_n"] == 11 for e in eb) and all(e["log_n"] in (10, 11) for e in eb)
    above = [e for e in eb if "rate_above_chunk" in e["classes"]]
    assert len(above) >= 3 and all((1 << e["rate_bits"]) > e["D"] for e in above)
    assert any(pc.num_chunks(e["R"], e["D"]) == 32 and e["D"] == 2 for e in eb) and any(e["C"] == 8 for e in eb)
    q = {e["name"]: e for e in eb if e["kind"] == "quotient"}
    assert q["quotient_alpha_0"]["alphas"] == [0, 0] and q["quotient_alpha_1"]["alphas"] == [1, 1]
    nc = q["quotient_noncanonical"]
    assert all(v >= P for v in nc["betas"] + nc["gammas"] + nc["alphas"])
    assert (B["proof_wires_p_minus_1"]()["wires"] == np.uint64(P - 1)).all()
    assert {(D, rb, n_gt, code) for _, _, D, _, rb, (n_gt, _), code in pc.REFUSALS_B} == {(16, 3, 0, -7), (8, 4, 0, -7), (2, 1, 3, -1)}


def prove_and_verify(e):
    op, fp = _oracle.plonk_params(e["R"], e["D"], e["C"]), pc.fri_params(e)
    pf = _oracle.plonk_perm_prove(e["wires"], e["sigmas"], e["log_n"], op, fp, digest=pc.DIGEST)
    cap = _oracle.Batch(e["sigmas"], e["log_n"], rate_bits=e["rate_bits"], cap_height=pc.FRI["cap_height"]).cap
    return pf, _oracle.plonk_perm_verify(pf, cap, op, fp, digest=pc.DIGEST)


@pytest.mark.parametrize("name", [n for n in pc.IDS_B if n.startswith("proof")])
def test_oracle_proofs_verify(name):
    """every whole-proof configuration of section B through the oracle's prover and verifier; the identity permutation's quotient is 0"""
    e = B[name]()
    pf, rc = prove_and_verify(e)
    assert rc == 0 and int(pf[1]) == e["log_n"] and [int(v) for v in pf[2:5]] == [e["R"], e["D"], e["C"]]
    if e["zero_quotient"]:
        assert (zero_quotient_chunks(e) == 0).all()


def zero_quotient_chunks(e):
    rng = np.random.default_rng(7)
    op = _oracle.plonk_params(e["R"], e["D"], e["C"])
    betas, gammas, alphas = ([int(v) for v in _oracle.rand_field(rng, (e["C"],))] for _ in range(3))
    zs = _oracle.plonk_zs(e["wires"], e["sigmas"], e["log_n"], op, betas, gammas)
    assert (zs == 1).all()
    co = [_oracle.Batch(a, e["log_n"], rate_bits=1, cap_height=0).coeffs for a in (e["wires"], e["sigmas"], zs)]
    return _oracle.plonk_quotient_chunks(co[0], co[1], co[2], e["log_n"], op, betas, gammas, alphas)


def test_gate_terms_entry_has_cells_that_fit_below_p():
    """the gate-term entry really has cells that can be handed over as value + p: gate 0's term is 0 on the whole quotient coset, gate
    1's is GATE_TERM_DEFECT, gate 2's (a satisfied gate on random wires) vanishes on the trace only; lifting changes the words, not the
    values"""
    e = B["quotient_gate_terms_plus_p"]()
    w = e["wires"].astype(object)
    assert ((w[0] * w[1] - w[2]) % P == 0).all() and ((w[3] * w[4] - w[5]) % P == pc.GATE_TERM_DEFECT).all() and ((w[6] * w[7] - w[8]) % P == 0).all()
    assert len(set(w[6].tolist())) > 100
    co = _oracle.Batch(e["wires"], e["log_n"], rate_bits=1, cap_height=0).coeffs
    nat = _oracle.plonk_gate_terms_coset(co, e["log_n"], e["D"].bit_length() - 1, e["num_mul"])
    assert (nat[0] == 0).all() and (nat[1] == pc.GATE_TERM_DEFECT).all() and (nat[2] >= (1 << 32) - 1).all()
    up = pc.lift(nat)
    assert (up[0] == P).all() and (up[1] == 2**64 - 1).all() and (up[2] == nat[2]).all()
    v = np.array([0, 1, (1 << 32) - 2, (1 << 32) - 1, P - 1], dtype=np.uint64)
    assert [int(x) for x in pc.lift(v)] == [P, P + 1, 2**64 - 1, (1 << 32) - 1, P - 1]
    assert (1 << e["rate_bits"]) > e["D"]
