"""The Python-integer reading of the lookup argument (tests/_lookup_cases.py) against its own statement, on the CPU: on every honest
entry the multiplicities make every term of the argument vanish on every row and the running sum S return to 0; one changed
multiplicity or one pair that is not in the table leaves a non-zero term; the catalogue reaches every edge class it names, checked on
the data and not on the labels alone.  The committed "SIPPPLK4" proof (tests/golden/lookup_proof_small.npz, written on a GPU by
tools/capture_lookup_fixture.py) through the library's host verifier, sipp_plonk_verify_gates_lookup, and the reading: accepted as it
is; refused with a flipped S opening, a changed header word, under another description, truncated.  And the host-only
sipp_plonk_lookup_num_columns."""
import ctypes as C

import numpy as np
import pytest

from tests import _lookup_cases as lc

P = lc.P


@pytest.fixture(scope="module")
def solved():
    """name -> (wires with the multiplicities, columns): computed once, read by every test below, never written"""
    out = {}
    for fn in lc.ENTRIES:
        e = fn()
        wires = lc.multiplicities(e["desc"], e["wires"], e["consts"])
        cols, closes = lc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])
        wires.setflags(write=False)
        cols.setflags(write=False)
        out[e["name"]] = (wires, cols, closes)
    return out


@pytest.mark.parametrize("name", lc.IDS)
def test_honest_entries_close_and_every_term_vanishes(solved, name):
    e = lc.BY_NAME[name]()
    wires, cols, closes = solved[name]
    J = len(lc.group_slots(e["desc"], e["D"]))
    assert cols.shape == (e["C"] * J, 1 << e["log_n"])
    assert closes, "S does not return to 0 around the subgroup"
    assert (cols[: e["C"], 0] == 0).all()
    assert lc.all_terms_vanish(e, wires, cols)


@pytest.mark.parametrize("name", ["n8_D2_look_D_tab_Dp1", "n64_D4_C8_look_2Dp3_tab_Dp1", "n4_one_table_row_one_looking_row"])
def test_one_changed_multiplicity_leaves_a_nonzero_term(solved, name):
    e = lc.BY_NAME[name]()
    tm = e["desc"][5]
    for delta in (1, P - 1):
        wires = solved[name][0].copy()
        i = e["table_rows"][0]
        wires[tm][i] = (int(wires[tm][i]) + delta) % P
        cols, closes = lc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])
        assert not closes
        assert not lc.all_terms_vanish(e, wires, cols)


def test_a_pair_outside_the_table_is_refused_and_leaves_a_nonzero_term(solved):
    e = lc.absent_pair()
    with pytest.raises(lc.Absent):
        lc.multiplicities(e["desc"], e["wires"], e["consts"])
    # with the multiplicities of the honest instance (the nearest a cheating prover gets) the sum no longer closes
    base = solved["n64_D4_C8_look_2Dp3_tab_Dp1"][0]
    tm, n_tab = e["desc"][5], e["desc"][6]
    wires = e["wires"].copy()
    wires[tm: tm + n_tab] = base[tm: tm + n_tab]
    cols, closes = lc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])
    assert not closes and not lc.all_terms_vanish(e, wires, cols)


@pytest.mark.parametrize("name", ["theta_on_a_looking_combination", "theta_on_a_table_combination"])
def test_theta_on_a_combination_is_refused(name):
    e = lc.BY_NAME[name]()
    wires = lc.multiplicities(e["desc"], e["wires"], e["consts"])
    with pytest.raises(lc.Vanishing):
        lc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])


def test_the_catalogue_reaches_every_edge_it_names(solved):
    reached = set()
    for fn in lc.ENTRIES + lc.SPOILED:
        reached |= fn()["classes"]
    assert reached == lc.EDGE_CLASSES
    shapes = {(e["D"], e["desc"][2], e["desc"][6]) for e in (fn() for fn in lc.ENTRIES)}
    assert {d for d, _, _ in shapes} == {2, 4, 8}
    assert {1} <= {nl for _, nl, _ in shapes} and any(nl == d for d, nl, _ in shapes) and any(nl == d + 1 for d, nl, _ in shapes)
    assert any(nl == 2 * d + 3 for d, nl, _ in shapes)
    assert any(nt == 1 for _, _, nt in shapes) and all(any(nt == d + 1 for d2, _, nt in shapes if d2 == d) for d in (2, 4, 8))
    assert {e()["C"] for e in lc.ENTRIES} == {1, 2, 8}
    assert {fn()["log_n"] for fn in lc.ENTRIES} >= {2, 10}
    for fn in lc.ENTRIES:
        e = fn()
        _, lw, n_look, q_tab, tc, tm, n_tab = lc.unpack(e["desc"])
        wires = solved[e["name"]][0]
        ms = {(k, i): int(wires[tm + k][i]) for i in e["table_rows"] for k in range(n_tab)}
        keys = {(k, i): (int(e["consts"][tc + 2 * k][i]), int(e["consts"][tc + 2 * k + 1][i])) for (k, i) in ms}
        assert sum(ms.values()) == len(e["look_rows"]) * n_look
        # the multiplicity cells of rows that are no table rows keep what they held
        others = [i for i in range(1 << e["log_n"]) if i not in e["table_rows"]]
        assert (wires[tm: tm + n_tab][:, others] == e["wires"][tm: tm + n_tab][:, others]).all()
        cl = e["classes"]
        if "never_hit" in cl:
            assert 0 in ms.values()
        if "one_entry" in cl:
            assert sorted(ms.values())[-1] == len(e["look_rows"]) * n_look
        if "padded_duplicates" in cl:
            seen = {}
            later = [ki for ki in sorted(ms, key=lambda ki: (ki[1], ki[0])) if seen.setdefault(keys[ki], ki) != ki]
            assert later and all(ms[ki] == 0 for ki in later)
        if "looks_on_duplicates" in cl:
            assert all(m == 0 or keys[ki] in e["repeated"] for ki, m in ms.items()) and any(ms.values())
        if "keys_ge_2_63" in cl:
            assert all(x >= 1 << 63 and y >= 1 << 63 for x, y in keys.values())
        if "words_plus_p" in cl:
            look = e["wires"][lw: lw + 2 * n_look][:, e["look_rows"]]
            assert (look >= np.uint64(P)).any() and e["etas"][0] >= P and e["thetas"][0] >= P
        if "row_both_table_and_looking" in cl:
            assert set(e["table_rows"]) & set(e["look_rows"])
        if "row0_marked" in cl:
            assert 0 in e["table_rows"] + e["look_rows"]
        if "last_row_marked" in cl:
            assert (1 << e["log_n"]) - 1 in e["table_rows"] + e["look_rows"]
        if "scan_several_rows_a_thread" in cl:
            assert 1 << e["log_n"] > 1024


# ---- the committed proof: tests/golden/lookup_proof_small.npz (tools/capture_lookup_fixture.py, written on the GPU) ---------------------
class Fixture:
    def __init__(self):
        import os
        import sipp_amd
        from sipp_amd.circuit import fri_params
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookup_proof_small.npz"))
        self.proof, self.cap = z["proof"], z["cap"]
        assert str(z["entry"]) == lc.PROOF_ENTRY
        self.e = e = lc.BY_NAME[lc.PROOF_ENTRY]()
        self.circ = sipp_amd.PlonkCircuit.from_dict(lc.proof_circuit(e))
        self.gp = sipp_amd.PlonkParams(lc.PROOF_ROUTED, e["D"], e["C"])
        self.fp = fri_params(e["log_n"], **lc.PROOF_FRI)
        self.proof.setflags(write=False)

    def verdict(self, proof, desc=None):
        import sipp_amd
        return sipp_amd.plonk_verify_gates_lookup(proof, self.cap, self.gp, self.fp, self.circ, lc.PROOF_DIGEST,
                                                  self.e["desc"] if desc is None else desc)

    def s_opening(self):
        """the word index of S_0(zeta).c0: behind the header, the three caps, the opening section's header, the constants, sigmas,
        wires and the permutation's columns"""
        e = self.e
        m = -(-lc.PROOF_ROUTED // e["D"])
        return 24 + 12 * (1 << lc.PROOF_FRI["cap_height"]) + 8 + 2 * (e["consts"].shape[0] + lc.PROOF_ROUTED + e["wires"].shape[0] + e["C"] * m)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_the_fixture_is_accepted_by_the_verifier_and_by_the_reading(fx):
    from sipp_amd.plonk_vanishing import _HostChallenger
    assert fx.e["log_n"] == 10 and fx.fp.num_queries == 8
    assert fx.verdict(fx.proof) == 0
    assert lc.read_proof(fx.proof, fx.e, _HostChallenger()) is None


def test_the_fixture_with_a_flipped_s_opening_is_refused(fx):
    from sipp_amd.plonk_vanishing import _HostChallenger
    for at in (fx.s_opening(), fx.s_opening() + 2 * fx.e["C"] - 1):         # S_0(zeta).c0, S_(C-1)(zeta).c1
        bad = fx.proof.copy()
        bad[at] ^= np.uint64(1)
        assert fx.verdict(bad) == 210, at
        assert lc.read_proof(bad, fx.e, _HostChallenger()) == "vanishing"
    # S_0(g zeta): the last C pairs of the opened values
    e = fx.e
    J = len(lc.group_slots(e["desc"], e["D"]))
    at = fx.s_opening() + 2 * (e["C"] * J + e["C"] * e["D"] + e["C"])
    bad = fx.proof.copy()
    bad[at] ^= np.uint64(1)
    assert fx.verdict(bad) == 210 and lc.read_proof(bad, fx.e, _HostChallenger()) == "vanishing"


@pytest.mark.parametrize("word", range(16, 24))
def test_the_fixture_with_a_changed_header_word_is_refused(fx, word):
    bad = fx.proof.copy()
    bad[word] += np.uint64(1)
    assert fx.verdict(bad) == 201


def test_the_fixture_under_another_description_is_refused(fx):
    d = list(fx.e["desc"])
    others = [d[:2] + [d[2] - 1] + d[3:], d[:6] + [d[6] - 1, 0], [d[3], d[1], d[2], d[0]] + d[4:], d[:1] + [d[1] - 1] + d[2:], [0] * 8]
    for desc in others:
        assert fx.verdict(fx.proof, desc) == 201, desc
    # a description that does not fit the circuit is refused whatever the proof says
    assert fx.verdict(fx.proof, [0] + d[1:]) == 201 and fx.verdict(fx.proof, d[:2] + [129] + d[3:]) == 201


def test_the_fixture_truncated_is_refused(fx):
    n = len(fx.proof)
    for keep in (1, 8, 23, 24, 24 + 12 * 16, fx.s_opening(), n // 2, n - 1):
        cut = fx.proof[:keep].copy()
        assert fx.verdict(cut) != 0, keep
        if keep > 5:
            cut[5] = keep          # even with the header's own length word adjusted
            assert fx.verdict(cut) != 0, keep


def test_num_columns_is_challenges_times_groups():
    """sipp_plonk_lookup_num_columns (host arithmetic, no GPU): C (ceil(n_look / D) + ceil(n_tab / D)); 0 for an empty description
    and for one outside the supported range"""
    import sipp_amd
    L = sipp_amd.lib()

    def ncols(D, Cn, desc):
        gp = sipp_amd.PlonkParams(1, D, Cn)
        return L.sipp_plonk_lookup_num_columns(C.byref(gp), (C.c_uint32 * 8)(*desc))

    for fn in lc.ENTRIES:
        e = fn()
        assert ncols(e["D"], e["C"], e["desc"]) == e["C"] * len(lc.group_slots(e["desc"], e["D"]))
    assert ncols(8, 2, (0,) * 8) == 0
    assert ncols(8, 2, (2, 0, 129, 3, 4, 4, 2, 0)) == 0 and ncols(8, 2, (2, 0, 2, 3, 4, 4, 129, 0)) == 0
    assert ncols(3, 2, lc.GOOD_DESC) == 0 and ncols(8, 9, lc.GOOD_DESC) == 0
    assert ncols(64, 8, (2, 0, 128, 3, 4, 4, 128, 0)) == 8 * 4
