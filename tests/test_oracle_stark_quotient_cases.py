"""The two CPU readings of the STARK constraints against each other on the crafted cells of tests/_stark_quotient_cases.py, the
catalogue's reach, and the oracle's Z stage against the cell-by-cell integer rule.  No GPU.

  orc_eval_base (oracle/air.c: air_eval.inc over the base field, through orc_quotient_points)
  eval_constraints (oracle/py/stark_verify.py: Python integers over the extension, fed the base point; periodic and value-periodic
  values, lagrange_first / lagrange_last / z_last and Z_H computed on the Python side)

must agree word for word at the sampled points of every case: eight leaf positions, among them both parities of the natural index and the
two points whose `next` row wraps.  The device is held against both in tests/test_gpu_stark_quotient_cases.py; this file makes sure that
what it is held against is one thing, and that the catalogue still reaches the edges it was built for (reached()).
"""
import numpy as np
import pytest

from tests import _oracle
from tests import _stark_quotient_cases as sq

P = sq.P


def _by_air():
    out = {}
    for case in sq.quotient_cases():
        out.setdefault(case.ai, []).append(case)
    return out


@pytest.mark.parametrize("ai", range(len(sq.AIRS)), ids=[a["name"] for a in sq.AIRS])
def test_two_readings_agree_on_every_case(ai):
    for case in _by_air()[ai]:
        lde, zlde, aux = sq.tables(case)
        assert all(int(t.max(initial=0)) < P for t in (lde, zlde, aux)), "a non-canonical cell in " + case.name
        ref = sq.check_two_readings(case, lde, zlde, aux, sq.sample_positions(case.log_n))
        if case.style == "zero" and not sq.refused(case):
            # all cells zero: not every constraint vanishes (Z - 1 on the first row, constants), so the values are not trivially zero
            assert ref.any(), case.name


BIG = sq.big_cases()


@pytest.mark.parametrize("case", BIG, ids=[c.name for c in BIG])
def test_two_readings_agree_at_log_n_15(case):
    """the g2_u16 tables at log_n = 15 are built on the device only; the readings take a gather of the sampled points and their next rows,
    built here from the same formula"""
    pos = sq.sample_positions(case.log_n)
    need, slot, (lde, zlde, aux) = sq.big_gather(case, pos)
    assert all(int(t.max(initial=0)) < P for t in (lde, zlde, aux)) and len(need) == 2 * len(pos) - 2   # m - 2 -> 0, m - 1 -> 1
    sq.check_two_readings(case, lde, zlde, aux, pos, slot)


def test_lattice_tables_show_every_value_to_every_class():
    case = next(c for c in sq.quotient_cases() if c.style == "lattice")
    lde, zlde, aux = sq.tables(case)
    cls = sq.lde_classes(sq.AIRS[case.ai])
    for k in range(5):
        col = lde[int(np.flatnonzero(cls == k)[0])]
        assert set(col.tolist()) == set(sq.LATTICE), "class %d" % k
    assert set(zlde[0].tolist()) == set(sq.LATTICE) and set(aux[0].tolist()) == set(sq.LATTICE)
    # leaf order: position j holds the formula's value at natural index bitrev(j)
    rev = sq.bitrev(case.log_n + 1)
    assert int(lde[3, 5]) == sq.LATTICE[int(sq.lattice_index(int(cls[3]), 3, int(rev[5])))]


def test_catalogue_reaches_what_it_was_built_for():
    r = sq.reached()
    cases = {c.name: c for c in sq.quotient_cases() + sq.big_cases()}
    name = lambda c: sq.AIRS[c.ai]["name"]
    # every entry of AIR_AIRS at its smallest trace, in every style
    for ai, a in enumerate(sq.AIRS):
        for style in sq.STYLES:
            assert any(c.ai == ai and c.style == style and c.log_n == sq.small_log_n(a) for c in cases.values()), (a["name"], style)
    assert len(sq.AIRS) == 14 and [sq.small_log_n(a) for a in sq.AIRS if a["kind"] == 6] == [13, 13]
    # the routes of quotient_rest: split everywhere at the small sizes but for pairing_u16 (63 checked columns); unsplit at log_n = 15
    for n, c in cases.items():
        want = "unsplit" if name(c) == "pairing_u16" or c.log_n == 15 else "split"
        assert r["route"][n] == want, n
    assert {r["route"][n] for n in cases} == {"split", "unsplit"}
    # an odd number of columns in a range: the min(k0 + u, nc - 1) clamp
    assert any(r["odd_clamp"][n] and r["route"][n] == "split" for n in cases) and any(r["odd_clamp"][n] and r["route"][n] == "unsplit" for n in cases)
    # RestAcc folds on the long unsplit walk only, and there in both big cases
    assert [n for n in cases if r["fold"][n]] == [c.name for c in sq.big_cases()]
    assert {c.style for c in sq.big_cases()} == {"pm1", "lattice", "fold"}
    # ... and in one of them it HAS to: without the fold a sum of F passes 2^64 (and wraps on the device), with it none does.  The case
    # is alpha = p - 1 with pin - ptab = Z - 1 = p - 1: 1134 terms of (2^32 - 1) x 0x3FFC00, the middle limb of p - 1, in sum 4
    assert {n: (kept < 1 << 64, bare >= 1 << 64) for n, (kept, bare) in r["fold_needed"].items()} == {
        "g2_u16@15-pm1": (True, False), "g2_u16@15-lattice": (True, False), "g2_u16@15-fold": (True, True)}
    assert r["fold_needed"]["g2_u16@15-fold"][1] == 1134 * (2 ** 32 - 1) * 0x3FFC00
    assert sq.limbs3(P - 1) == (0, 0x3FFC00, 0xFFFFF) and cases["g2_u16@15-fold"].alpha == (P - 1, P - 1)
    # the sliced gadget: the pairing AIRs
    assert {name(cases[n]) for n in cases if r["sliced"][n]} == {"pairing_u16", "pairing_u8"}
    # the q * p carry fires in EVERY gadget of every AIR (hence of every family) in the `carry` style, at the coefficient it was solved for
    fams = set()
    for n, fired in r["carry"].items():
        c = cases[n]
        for gi in range(len(sq.gadgets(c.ai)[0])):
            assert (gi, sq.craft_q(c.ai, gi)[1]) in fired, (n, gi)
        fams.add(sq.family(sq.AIRS[c.ai]))
    assert fams == set(sq.FAMILIES) and len(r["carry"]) == len(sq.AIRS)
    # the three paths of the lazy POLY fold in every AIR
    for air, cnt in r["poly_coefficients"].items():
        assert all(cnt[k] > 0 for k in ("+1", "-1", "other")), (air, cnt)
    # refusals: alpha = 0 in either component
    assert sorted(c.alpha.index(0) for c in cases.values() if sq.refused(c)) == [0, 1]
    # Z: <4> in one block and in several, <8>, and more than 256 blocks (both chunk loops of z_phase_b cross a chunk)
    z = {c.name: c for c in sq.z_cases()}
    assert {(r["z_rows"][n], min(r["z_blocks"][n], 2)) for n in z} == {(4, 1), (4, 2), (8, 2)}
    assert any(r["z_chunk_loop"][n] for n in z) and all(z[n].log_n == 20 for n in z if r["z_chunk_loop"][n])
    assert any(c.nc == sq.AIRS[sq.G1_U8]["n_checked"] for c in z.values())
    for tag in ("row0", "last", "lane", "block", "twice"):
        assert any(("den=0@" + tag) in n for n in z), tag
    assert sq.rest_folds(15, 320) == 1 and sq.rest_folds(15, 318) == 0       # the threshold as the kernel has it


def test_carry_model_is_the_kernels():
    # the model against plain integer multiplication: (h, l) with the carry is the exact 96-bit sum, without it is 2^64 short
    for ai in (0, 9, 13):
        for gi in range(len(sq.gadgets(ai)[0])):
            q, k = sq.craft_q(ai, gi)
            assert all(v < P for v in q) and k in sq.qp_carries(q)
            exact = sum(q[i] * sq.P_LIMBS[k - i] for i in range(17) if 0 <= k - i < 16)
            al = sum((q[i] & sq.M32) * sq.P_LIMBS[k - i] for i in range(17) if 0 <= k - i < 16)
            ah = sum((q[i] >> 32) * sq.P_LIMBS[k - i] for i in range(17) if 0 <= k - i < 16)
            lo = (al + (ah << 32)) & sq.M64
            assert ((ah >> 32) + 1) << 64 | lo == exact


# ---------------------------------------------------------------------------------------------------- Z
SMALL_Z = [c for c in sq.z_cases() if c.log_n <= 14]


@pytest.mark.parametrize("case", SMALL_Z, ids=[c.name for c in SMALL_Z])
def test_oracle_z_columns_follow_the_cell_rule(case):
    trace = sq.z_trace(case)
    want = sq.z_reference(case, trace)
    got = _oracle.z_columns(trace, case.n_main, case.cbase, case.nc, case.beta, case.gamma)
    assert (got == want).all(), "%s: orc_z_columns leaves the cell-by-cell rule in column(s) %s" % (case.name, np.flatnonzero((got != want).any(axis=1))[:8])
    if "den=0" in case.name:
        # the rule, spelled out: every patched column is zero after its FIRST vanishing denominator and untouched up to it
        first = {}
        for what, j, i, r in case.patches:
            first[i * case.nc + j] = min(r, first.get(i * case.nc + j, r))
        assert len(first) == 2
        for zi, r in first.items():
            assert want[zi, 0] == 1 and not want[zi, r + 1:].any() and (r == 0 or want[zi, 1:r + 1].all())


def test_oracle_z_relation_at_two_to_the_twenty():
    for case in (c for c in sq.z_cases() if c.log_n == 20):
        trace = sq.z_trace(case)
        got = _oracle.z_columns(trace, case.n_main, case.cbase, case.nc, case.beta, case.gamma)
        assert sq.z_relation_holds(case, trace, got), case.name
