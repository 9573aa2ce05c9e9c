"""The tagged reading of the lookup argument (tests/_lookup_tables_cases.py) against its own statement, on the CPU: on every honest
entry the multiplicities make every term vanish on every row and S return to 0; a tag flipped on one looking row, and a multiplicity
moved to the equal pair under the other tag, leave a non-zero term; the catalogue reaches every edge class it names, checked on the
data; the generator's integer rule on its instances.  The committed two-table "SIPPPLK4" proof
(tests/golden/lookup_tables_proof_small.npz, written on a GPU by tools/capture_lookup_tables_fixture.py) through the library's host
verifier and the reading: accepted as it is; refused with 201 when word 7 of the caller's description differs, with 210 when an
opened tag value is flipped."""
import numpy as np
import pytest

from tests import _lookup_cases as lc
from tests import _lookup_tables_cases as tc

P = tc.P


@pytest.fixture(scope="module")
def solved():
    """name -> (wires with the multiplicities, columns, closes): computed once, never written"""
    out = {}
    for fn in tc.ENTRIES:
        e = fn()
        wires = tc.multiplicities(e["desc"], e["wires"], e["consts"])
        cols, closes = tc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])
        wires.setflags(write=False)
        cols.setflags(write=False)
        out[e["name"]] = (wires, cols, closes)
    return out


@pytest.mark.parametrize("name", tc.IDS)
def test_honest_entries_close_and_every_term_vanishes(solved, name):
    e = tc.BY_NAME[name]()
    wires, cols, closes = solved[name]
    J = len(tc.group_slots(e["desc"], e["D"]))
    assert cols.shape == (e["C"] * J, 1 << e["log_n"])
    assert closes and (cols[: e["C"], 0] == 0).all()
    assert tc.all_terms_vanish(e, wires, cols)
    # the tags are what makes them vanish: read without them (one table), the same columns leave a term
    one = dict(e, desc=e["desc"][:7] + (0,))
    assert not lc.all_terms_vanish(one, wires, cols)


def test_a_tag_flipped_on_one_looking_row_leaves_a_nonzero_term(solved):
    e = tc.tag_flipped_on_a_looking_row()
    with pytest.raises(tc.Absent):
        tc.multiplicities(e["desc"], e["wires"], e["consts"])
    # with the honest instance's multiplicities (the nearest a cheating prover gets)
    wires = solved["n8_D2_straddle_C8_shared"][0]
    cols, closes = tc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])
    assert not closes and not tc.all_terms_vanish(e, wires, cols)


@pytest.mark.parametrize("name", ["n8_D2_straddle_C8_shared", "n16_big_tags_and_words_plus_p", "n4_one_row_each"])
def test_a_multiplicity_moved_to_the_other_tag_leaves_a_nonzero_term(solved, name):
    """entry 0 of table 0 gives one of its looks to a slot of table 1: where the pair is shared, to the EQUAL pair under the other tag"""
    e = tc.BY_NAME[name]()
    tm, n_tab = e["desc"][5], e["desc"][6]
    wires = solved[name][0].copy()
    i0, i1 = e["tables"][0][2][0], e["tables"][1][2][0]
    if "same_pair_under_both_tags" in e["classes"]:
        tcol = e["desc"][4]
        assert (e["consts"][tcol][i0], e["consts"][tcol + 1][i0]) == (e["consts"][tcol][i1], e["consts"][tcol + 1][i1])
    assert int(wires[tm][i0]) >= 1
    wires[tm][i0] -= np.uint64(1)
    wires[tm][i1] += np.uint64(1)
    cols, closes = tc.sums(e["desc"], wires, e["consts"], e["D"], e["etas"], e["thetas"])
    assert not closes and not tc.all_terms_vanish(e, wires, cols)
    if "same_pair_under_both_tags" in e["classes"]:      # read as one table the two slots are one entry: the sum closes again
        one = e["desc"][:7] + (0,)
        assert lc.sums(one, wires, e["consts"], e["D"], e["etas"], e["thetas"])[1]


def test_a_pair_only_under_the_other_tag_is_absent():
    e = tc.pair_only_under_the_other_tag()
    with pytest.raises(tc.Absent):
        tc.multiplicities(e["desc"], e["wires"], e["consts"])
    lc.multiplicities(e["desc"][:7] + (0,), e["wires"], e["consts"])          # as one table it is there


def test_the_catalogue_reaches_every_edge_it_names(solved):
    reached = set()
    for fn in tc.ENTRIES + tc.SPOILED:
        reached |= fn()["classes"]
    assert reached == tc.EDGE_CLASSES
    for fn in tc.ENTRIES:
        e = fn()
        q_look, lw, n_look, q_tab, tcol, tm, n_tab, tag0 = e["desc"]
        wires = solved[e["name"]][0]
        n, cl, D = 1 << e["log_n"], e["classes"], e["D"]
        assert tag0 and len(e["tables"]) >= 2
        assert int(wires[tm: tm + n_tab][:, e["table_rows"]].sum()) == len(e["look_rows"]) * n_look
        # garbage in the tag columns of unmarked rows
        unmarked = [i for i in range(n) if i not in e["look_rows"]]
        assert len(set(int(v) for v in e["consts"][tag0][unmarked])) > 1 or len(unmarked) <= 1
        if "n4_single_rows" in cl:
            assert n == 4 and all(len(t[2]) == 1 and len(t[3]) == 1 for t in e["tables"])
        if "groups_straddle" in cl:
            assert n_look % D and n_look > D and n_tab % D and n_tab > D
        if "eight_challenges" in cl:
            assert e["C"] == 8
        if "three_tables" in cl:
            assert len({t[0] % P for t in e["tables"]}) == 3
        if "same_pair_under_both_tags" in cl:
            # the shared pair has a count under EVERY tag: the counts split by tag and do not all go to the first slot
            for t in e["tables"]:
                i = t[2][0]
                assert (int(e["consts"][tcol][i]), int(e["consts"][tcol + 1][i])) == e["entries"][0][0] and int(wires[tm][i]) >= len(t[3])
        if "tags_ge_2_63" in cl:
            assert any(t[0] % P >= 1 << 63 for t in e["tables"])
        if "tag_words_plus_p" in cl:
            assert any(t[0] >= P or t[1] >= P for t in e["tables"]) and any(t[0] != t[1] for t in e["tables"])
        if "several_blocks" in cl:
            assert n > 256
        if "row0_marked" in cl:
            assert 0 in e["table_rows"] + e["look_rows"]
        if "last_row_marked" in cl:
            assert n - 1 in e["table_rows"] + e["look_rows"]


def test_the_generator_rule_on_its_instances():
    """the integer reading of SIPP_GEN_LOOKUP, value by value on the small instance"""
    e = tc.gen_n8()
    w, x = e["expected"], e["wires"]
    assert [int(w[2][3]), int(w[4][3])] == [(1 << 63) + 11, (1 << 63) + 3]          # x = 0, x = T - 1
    assert [int(w[2][4]), int(w[4][4])] == [0, P - 1]                                # x = T; x = 3 + p under row0 = 0 + p
    assert [int(w[2][5]), int(w[4][5])] == [6, 0]                                    # g(3); g's entry 6 would sit in row N
    assert (w[:, 2] == x[:, 2]).all() and int(x[2][2]) == tc.SENTINEL                # the T = 0 row, byte for byte
    assert int(e["consts"][6][1]) == 17 + P and tc.generate(x, e["consts"], [(tc.GEN_LOOKUP, 0, 1, 1, 1, 3, 3, 1)])[0][2][3] == w[2][3]
    assert int(e["written"].sum()) == 6 and ((w != x) <= e["written"]).all()
    c = tc.gen_n8_chain()["expected"]
    assert [int(c[2][3]), int(c[4][3]), int(c[2][4]), int(c[4][4]), int(c[2][6]), int(c[4][6])] == [4, 1, 5, 3, 1, 3]
    wide = tc.gen_wide_level()
    rows = np.flatnonzero(wide["consts"][0] == 1)
    assert len(rows) > 7000 and (wide["wires"][1][rows] >= 256).any() and (wide["expected"][2][rows][wide["wires"][1][rows] >= 256] == 0).all()


# ---- the committed proof ---------------------------------------------------------------------------------------------------------------
class Fixture:
    def __init__(self):
        import os
        import sipp_amd
        from sipp_amd.circuit import fri_params
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookup_tables_proof_small.npz"))
        self.proof, self.cap = z["proof"], z["cap"]
        assert str(z["entry"]) == tc.PROOF_ENTRY
        self.e = e = tc.BY_NAME[tc.PROOF_ENTRY]()
        self.circ = sipp_amd.PlonkCircuit.from_dict(lc.proof_circuit(e))
        self.gp = sipp_amd.PlonkParams(lc.PROOF_ROUTED, e["D"], e["C"])
        self.fp = fri_params(e["log_n"], **lc.PROOF_FRI)
        self.proof.setflags(write=False)

    def verdict(self, proof, desc=None):
        import sipp_amd
        return sipp_amd.plonk_verify_gates_lookup(proof, self.cap, self.gp, self.fp, self.circ, lc.PROOF_DIGEST,
                                                  self.e["desc"] if desc is None else desc)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def reading(proof, e):
    from sipp_amd.plonk_vanishing import _HostChallenger
    return tc.read_proof(proof, e, _HostChallenger())


def test_the_fixture_is_accepted_by_the_verifier_and_by_the_reading(fx):
    assert fx.e["log_n"] == 10 and fx.fp.num_queries == 8 and len(fx.proof) < 4096
    assert [int(v) for v in fx.proof[16:24]] == list(fx.e["desc"]) and fx.e["desc"][7] != 0
    assert fx.verdict(fx.proof) == 0
    assert reading(fx.proof, fx.e) is None


def test_the_fixture_under_another_word_7_is_refused_with_201(fx):
    d = fx.e["desc"]
    for word7 in (0, d[7] - 1, d[7] + 1, d[0], 0xFFFFFFFF):
        assert fx.verdict(fx.proof, d[:7] + (word7,)) == 201, word7
    bad = fx.proof.copy()
    bad[23] = 0                                        # the header's own word 7 against the caller's
    assert fx.verdict(bad) == 201 and fx.verdict(bad, d[:7] + (0,)) != 0


def test_the_fixture_with_a_flipped_tag_opening_is_refused_with_210(fx):
    at = tc.tag_opening(fx.e)
    for k in (at, at + 1, at + 2, at + 3):             # the looking rows' tag column, then the table rows', c0 and c1
        bad = fx.proof.copy()
        bad[k] ^= np.uint64(1)
        assert fx.verdict(bad) == 210, k
        assert reading(bad, fx.e) == "vanishing"


def test_the_reading_without_the_tag_term_refuses_the_fixture(fx):
    """the untagged reading's equation does not hold at zeta: the tag term is in the proof"""
    from sipp_amd.plonk_vanishing import _HostChallenger
    assert lc.read_proof(fx.proof, fx.e, _HostChallenger()) == "vanishing"
