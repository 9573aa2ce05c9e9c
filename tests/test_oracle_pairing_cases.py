"""The catalogue of pairing products tests/_pairing_cases.py against itself and the CPU readings (no GPU): it reaches the edges it
names, its two kinds of expectation (bn.multi_pairing / the closed form e(G1, G2)^(sum a_i b_i)) agree where both can be computed, the
Python pairing agrees with the C reading of the pairing AIR's schedule (oracle/pairing.c) on every finite single pair, and the Python
verifier runs on the crafted and tampered proofs -- its verdicts and statements are what tests/test_gpu_pairing_edges.py holds the
device against."""
import numpy as np
import pytest

from oracle.py import bn254 as bn
from tests import _oracle
from tests import _pairing_cases as PC

P = bn.P


def test_the_catalogue_reaches_its_edges():
    cases = PC.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    g1 = [a for c in cases for g in c.groups for a, _ in g if a is not None]
    assert any(x < 1 << 16 for x, _ in g1) and any(P - x < 1 << 16 for x, _ in g1)        # a coordinate next to 0 and next to p
    assert (1, P - 2) in g1                                                                   # -G1
    assert any(x >> 240 == 0x3063 and x & ((1 << 240) - 1) > (1 << 240) - (1 << 16) for x, _ in g1)   # fifteen 0xFFFF limbs
    assert all(bn.g1_on_curve(a) for a in set(g1))
    g2 = {b for c in cases for g in c.groups for _, b in g if b is not None}
    assert all(bn.g2_on_curve(b) for b in g2)
    assert all(bn.g2_mul(b, bn.R) is None for b in list(g2)[:: max(1, len(g2) // 16)])       # (a sample: points of G2, not just of the twist)
    # each infinity shape: alone, first and last in a small group, and inside the size cases at 0, 255, 256, n - 1
    shape = lambda a, b: "g1" if a is None and b is not None else "g2" if b is None and a is not None else "both" if a is None else None
    for s in PC.INF_SHAPES:
        assert any(len(c.groups[0]) == 1 and shape(*c.groups[0][0]) == s for c in cases)
        assert any(len(c.groups[0]) == 3 and shape(*c.groups[0][0]) == s and shape(*c.groups[0][1]) is None for c in cases)
        assert any(len(c.groups[0]) == 3 and shape(*c.groups[0][2]) == s and shape(*c.groups[0][1]) is None for c in cases)
        assert any(len(c.groups[0]) > 255 and s in {shape(*pq) for pq in c.groups[0]} for c in cases)
    sizes = {len(c.groups[0]) for c in cases}
    assert set(PC.SIZES) | {1, 2, 3, 4, 5, 6, 7} <= sizes
    for n in PC.SIZES:
        c = next(c for c in cases if c.name == "size_%d_with_inf" % n)
        assert {i for i, pq in enumerate(c.groups[0]) if shape(*pq)} == {0, 255, 256, n - 1} & set(range(n))
    for n in (257, 513):
        c = next(c for c in cases if c.name == "lone_pair_of_%d" % n)
        assert [i for i, pq in enumerate(c.groups[0]) if shape(*pq) is None] == [n - 1]
    assert {(len(c.groups), len(c.groups[0])) for c in cases if len(c.groups) > 1} == {(3, 257), (5, 257), (7, 1)}
    for c in cases:                                                                           # a group that reads its neighbour's slot is seen
        assert len({tuple(w) for w in c.want}) == len(c.want)


def test_recorded_expectations_are_the_computed_ones():
    """tests/golden/pairing_small_cases.npz, which the GPU test reads instead of computing 45 final exponentiations in Python again"""
    computed, recorded = PC.small_cases(), PC.small_cases_recorded()
    assert [c.name for c in recorded] == [c.name for c in computed]
    for c, r in zip(computed, recorded):
        assert r.groups == c.groups and r.want == c.want, c.name


def test_expectations_that_are_known_without_a_pairing():
    by = {c.name: c for c in PC.small_cases()}
    for name in ("only_inf_g1_n1", "only_inf_g2_n1", "only_inf_both_n1", "only_inf_n3", "cancel_negp", "cancel_negq", "cancel_scalar"):
        assert by[name].want == [bn.F12_ONE], name
        assert PC.case_words(by[name])[3].tolist() == [[1] + [0] * 95]
    e = by["g1_g2"].want[0]
    assert e != bn.F12_ONE and bn.f12_pow(e, bn.R) == bn.F12_ONE
    assert by["negg1_g2"].want[0] == by["g1_negg2"].want[0] == by["srm1_on_g1"].want[0] == by["srm1_on_g2"].want[0] == bn.f12_pow(e, bn.R - 1)
    assert by["s2_on_g1"].want[0] == by["s2_on_g2"].want[0] == bn.f12_mul(e, e)
    assert bn.f12_mul(by["shalf_on_g1"].want[0], by["shalf_on_g2"].want[0]) == e
    rep = by["repeat_4"]
    assert rep.want[0] == bn.f12_pow(bn.pairing(*rep.groups[0][0]), 4)
    for shape in PC.INF_SHAPES:                                     # the infinity pair contributes nothing, wherever it stands
        assert by["inf_%s_first_of_3" % shape].want == by["inf_%s_last_of_3" % shape].want == by["inf_g1_first_of_3"].want
    # infinity words are all zero, on the side the shape names only
    g1, g2, _, _ = PC.case_words(by["only_inf_n3"])
    assert [bool(g1[i].any()) for i in range(3)] == [False, True, False] and [bool(g2[i].any()) for i in range(3)] == [True, False, False]


def test_closed_form_equals_multi_pairing():
    """the size cases' expectation against Miller loops, at the one size (8) where the latter is affordable, and with infinity pairs"""
    A, B, _, _ = PC.chain()
    pairs, want = PC.chain_group(0, 8)
    assert pairs == list(zip(A[:8], B[:8]))
    assert want == bn.multi_pairing(A[:8], B[:8])
    pairs, want = PC.chain_group(257, 262, {0: "g1", 3: "g2", 4: "both"})
    assert [a is None for a, _ in pairs] == [True, False, False, False, True] and [b is None for _, b in pairs] == [False, False, False, True, True]
    assert want == bn.multi_pairing([a for a, _ in pairs], [b for _, b in pairs]) == bn.multi_pairing(A[258:260], B[258:260])
    # and the ragged small cases (exact) against the closed form
    for n in (3, 5, 6, 7):
        c = next(c for c in PC.small_cases() if c.name == "ragged_n%d" % n)
        assert c.want[0] == PC.chain_group(0, n)[1]


def test_chain_points_are_the_multiples_they_claim():
    A, B, a, b = PC.chain()
    for i in (0, 1, 255, 256, 512, PC.CHAIN_LEN - 1):
        assert A[i] == bn.g1_mul(bn.G1, a[i]) and B[i] == bn.g2_mul(bn.G2, b[i])
    assert len(set(A)) == len(A) and len(set(B)) == len(B)


def test_python_pairing_equals_the_c_reading_on_single_pairs():
    by = {c.name: c for c in PC.small_cases()}
    for name, a, b in PC.single_pairs():
        got = _oracle.pairing(np.array(PC.g1_words(a) + PC.g2_words(b), dtype=np.uint32))
        assert got.tolist() == bn.f12_to_u32(by[name].want[0]), name
    # the C reading has no infinity (the pairing AIR has no witness for it): it refuses with -2, the catalogue does not use it there
    L = _oracle.load()
    out = np.zeros(96, dtype=np.uint32)
    L.orc_pairing.argtypes = [_oracle.u32p, _oracle.u32p]
    for shape in PC.INF_SHAPES:
        a, b = PC.infinity(shape, bn.G1, bn.G2)
        assert L.orc_pairing(np.array(PC.g1_words(a) + PC.g2_words(b), dtype=np.uint32), out) == -2, shape


def test_python_verifier_on_crafted_proofs():
    els = PC.provable_elements()
    assert [n for n, _ in els] == ["one", "all_pm1", "all_top", "w6", "alt_pm1_0", "c11_pm1", "all_2p240", "base_field", "field_values"]
    used = set()
    for name, n, proof in PC.crafted_proofs():
        assert len(proof) == 2 * (n.bit_length() - 1) + 1
        used |= set(proof)
        ok, st, (g1, g2, f12) = PC.python_reading(*PC.crafted_points(n), proof)
        assert ok is False, name
        assert st.shape == (48 * n + 240,) and g1.shape == (n - 1, 56) and g2.shape == (n - 1, 104) and f12.shape == (2 * (n.bit_length() - 1), 296)
        assert st[48 * n: 48 * n + 96].tolist() == bn.f12_to_u32(list(proof[-1]))                # Z is the message sent first
        assert all(c < P for c in PC.f12_of([int(x) for x in st[-96:]]))
    assert used == {tuple(v) for _, v in els}
    n, proof = PC.zero_message_proof()
    ok, st, _ = PC.python_reading(*PC.crafted_points(n), proof)
    assert ok is False and not st[-96:].any()                                                   # Z Z_L^x = 0 stays 0


def test_python_verifier_on_the_tamper_table():
    A, B, honest = PC.fixture(8)
    d = np.load("tests/golden/sipp_n8_ios.npz")
    ok, st, ios = PC.python_reading(A, B, honest)
    assert ok and (st == d["statement"]).all() and all((g == d[k]).all() for g, k in zip(ios, ("g1", "g2", "fq12")))
    table = PC.tampered_proofs()
    assert len(table) == 14 and {m for _, m, _ in table} == set(range(7))
    for name, m, pf in table:
        diff = np.argwhere(pf != honest)
        assert diff.tolist() == [[m, 0 if name.startswith("low") else 95]], name
        assert bin(int(pf[tuple(diff[0])]) ^ int(honest[tuple(diff[0])])).count("1") == 1
    by = {name: pf for name, _, pf in table}
    for name in PC.READ_TAMPERED:
        ok, st2, _ = PC.python_reading(A, B, by[name])
        assert ok is False, name
        assert (st2[: 48 * 8] == st[: 48 * 8]).all() and (st2[-96:] != st[-96:]).any()


@pytest.mark.parametrize("top,want", [(0, 1), (1, 0), (0x30644E72, 0x10644E72), (0x2FFFFFFF, 0x0FFFFFFF), (0x00010000, 0)])
def test_flip_top_limb_changes_one_bit_downwards_or_sets_the_lowest(top, want):
    assert PC.flip_top_limb(top) == want
