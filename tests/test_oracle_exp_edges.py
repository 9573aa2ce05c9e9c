"""The exponentiation AIRs (G1 / G2 / Fq12 and the hardened G1 / G2) on the CPU oracle over the edge catalogue tests/_exp_edges.py:
every row of every trace satisfies its constraints; a Python-integer double-and-add / square-and-multiply follows every record through its
512 rows and pins the oracle's state cells; the `refused` records are refused by exactly the variants the catalogue names; the catalogue
reaches the edges it is meant for (both signs, zero quotients, constant columns, the hardened limb search at limb 0 and the last limb); the
gadgets' declared bounds (tools/air_gen.py bound_bits) hold by interval arithmetic over the programs of all seven AIRs; data/air_tables.h
is what the generator writes."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from oracle.py import bn254 as bn
from tests import _exp_edges as E
from tests import _oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "tools")):      # (the generator imports map_to_g2 / bn254 by bare name)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import air_gen  # noqa: E402

P = bn.P
GL = 2**64 - 2**32 + 1


def arr(kind, recs):
    return np.array(E.words(kind, recs), dtype=np.uint32)


@functools.lru_cache(maxsize=2)
def trace_of(kind):
    return _oracle.Trace(kind, arr(kind, E.records(kind)))


@functools.lru_cache(None)
def air_of(kind, mode="u8"):
    if kind == 2:
        return air_gen.build_fq12(mode)
    return air_gen.build_curve("g%d" % (kind % 4 + 1), mode, kind % 4 + 1, hardened=kind >= 4)


def failing_rows(t, rows=None):
    """the rows on which check_row names a constraint; the calls are independent (the trace is only read) and leave the interpreter's lock"""
    from concurrent.futures import ThreadPoolExecutor
    rows = list(range(1 << t.log_n) if rows is None else rows)
    nthr = max(1, min(8, len(os.sched_getaffinity(0))))
    chunks = [rows[i::nthr] for i in range(nthr)]
    with ThreadPoolExecutor(nthr) as ex:
        bad = ex.map(lambda ch: [r for r in ch if t.check_row(r) != -1], chunks)
    return sorted(r for b in bad for r in b)


def limbs_to_bytes(a, base, ncells, bits):
    """cells [base, base + ncells) of every row as one little-endian byte string per row: [n][ncells * bits / 8]"""
    return np.ascontiguousarray(a[base: base + ncells].astype("<u2" if bits == 16 else "u1").T).view(np.uint8)


def fq_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


# ---------------- every row, every kind ----------------
@pytest.mark.parametrize("kind", [0, 4, 1, 5, 2])
def test_every_row_of_the_catalogue_trace_holds(kind):
    """the trace builds (so every claimed output, computed in Python, is the chain's: a wrong one is refused with -8) and check_row passes on
    EVERY row, padding blocks included"""
    t = trace_of(kind)
    assert t.air.table_bits == 8 and t.num_io >= len(E.records(kind))
    bad = failing_rows(t)
    assert not bad, "kind %d: rows %s (records %s)" % (kind, bad[:8], sorted({E.records(kind)[min(r >> 9, len(E.records(kind)) - 1)].name for r in bad})[:4])


# ---------------- the third reading: Python integers through the 512 rows ----------------
def curve_chain(kind, rec):
    """(Rx, Ry, Px, Py, lam, X3, Y3) per row, each a tuple of Fq components, by the AIR's rules (tools/air_gen.py build_curve)"""
    if kind == 0:
        sub, mul, inv, c = (lambda a, b: (a - b) % P), (lambda a, b: a * b % P), bn.inv, (lambda a: (a,))
        k3, k2 = 3, 2
    else:
        sub, mul, inv, c = bn.f2_sub, bn.f2_mul, bn.f2_inv, (lambda a: a)
        k3, k2 = (3, 0), (2, 0)
    Rp, Pp = rec.off, rec.x
    rows = []
    for r in range(512):
        if r % 2 == 0:
            lam = mul(sub(Pp[1], Rp[1]), inv(sub(Pp[0], Rp[0])))
            xa, ya, xb = Rp[0], Rp[1], Pp[0]
        else:
            lam = mul(mul(k3, mul(Pp[0], Pp[0])), inv(mul(k2, Pp[1])))
            xa, ya, xb = Pp[0], Pp[1], Pp[0]
        x3 = sub(sub(mul(lam, lam), xa), xb)
        y3 = sub(mul(lam, sub(xa, x3)), ya)
        rows.append(tuple(c(v) for v in (Rp[0], Rp[1], Pp[0], Pp[1], lam, x3, y3)))
        if r % 2 == 0:
            if (rec.e >> (r // 2)) & 1:
                Rp = (x3, y3)
        elif r != 511:
            Pp = (x3, y3)
    return rows, Rp


@pytest.mark.parametrize("kind", [0, 1])
def test_python_double_and_add_pins_the_state_cells_of_the_curve_traces(kind):
    recs = E.records(kind)
    t = trace_of(kind)
    a, air = t.array(), air_of(kind)
    ext = kind + 1
    nrows = 512 * len(recs)
    want = [[] for _ in range(7)]
    for rec in recs:
        rows, out = curve_chain(kind, rec)
        assert out == rec.out, rec.name                     # the chain's result is the catalogue's offset + [e] x (another route: bn.g*_mul)
        for row in rows:
            for k in range(7):
                want[k].append(fq_bytes(row[k]))
    for k, nm in enumerate(("Rx", "Ry", "Px", "Py", "lam", "X3", "Y3")):
        checked = k >= 4
        got = limbs_to_bytes(a, air.col(nm), 16 * ext * (2 if checked else 1), 8 if checked else 16)[:nrows]
        exp = np.frombuffer(b"".join(want[k]), dtype=np.uint8).reshape(nrows, 32 * ext)
        bad = np.argwhere((got != exp).any(axis=1))
        assert bad.size == 0, "%s differs from the integers on rows %s (record %s)" % (nm, bad[:4, 0].tolist(), recs[int(bad[0, 0]) >> 9].name)


def tower(c):
    out = []
    for i in range(6):
        out += [(c[i] + 9 * c[i + 6]) % P, c[i + 6]]
    return out


def test_python_square_and_multiply_pins_the_state_cells_of_the_fq12_trace():
    recs = E.records(2)
    t = trace_of(2)
    a, air = t.array(), air_of(2)
    nrows = 512 * len(recs)
    want = [[], [], []]
    for rec in recs:
        acc, pw = rec.off, rec.x
        for r in range(512):
            c = bn.f12_mul(acc, pw) if r % 2 == 0 else bn.f12_mul(pw, pw)
            for k, v in enumerate((acc, pw, c)):
                want[k].append(fq_bytes(tower(v)))
            if r % 2 == 0:
                if (rec.e >> (r // 2)) & 1:
                    acc = c
            elif r != 511:
                pw = c
        assert acc == rec.out, rec.name
    for k, nm in enumerate(("acc", "pw", "C")):
        got = limbs_to_bytes(a, air.col(nm), 12 * 16 * (2 if k == 2 else 1), 8 if k == 2 else 16)[:nrows]
        exp = np.frombuffer(b"".join(want[k]), dtype=np.uint8).reshape(nrows, 12 * 32)
        bad = np.argwhere((got != exp).any(axis=1))
        assert bad.size == 0, "%s differs from the integers on rows %s (record %s)" % (nm, bad[:4, 0].tolist(), recs[int(bad[0, 0]) >> 9].name)


# ---------------- refusal ----------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_refused_records_are_refused_by_the_variants_the_catalogue_names(kind):
    good = E.records(kind)
    proved = {kind: [], kind + 4: []}
    for ref in E.refused(kind):
        batch = [good[0], ref, good[1]]
        for k, no_witness in ((kind, ref.plain),) + (((kind + 4, ref.hardened),) if kind < 2 else ()):
            if no_witness:
                with pytest.raises(RuntimeError):
                    _oracle.Trace(k, arr(k, batch))
            else:
                t = _oracle.Trace(k, arr(k, batch))
                assert not failing_rows(t), (ref.name, k)
                proved[k].append(ref)
    assert not proved[kind]                                  # every entry is refused by the plain AIR at least
    if kind < 2:                                             # what the hardened AIR proves instead: one proof over all of them
        assert len(proved[kind + 4]) == 4
        pf = _oracle.stark_prove(kind + 4, arr(kind, proved[kind + 4]))
        assert _oracle.stark_verify(pf) == 0
        with pytest.raises(RuntimeError):
            _oracle.stark_prove(kind, arr(kind, proved[kind + 4]))


# ---------------- what the catalogue must reach ----------------
def gadget_cells(t, air, g):
    """(sign [n], quotient limbs [17][n], carries [15][n] as signed integers) of gadget g over the trace"""
    a = t.array()
    nm = g["name"]
    sign = a[air.col(nm + "_s")]
    qb = air.col(nm + "_q")
    q = np.stack([a[qb + 2 * i] + 256 * a[qb + 2 * i + 1] for i in range(air_gen.NQ)]) if air.cpl == 2 else a[qb: qb + air_gen.NQ]
    cb, ncl, lb = air.col(nm + "_c"), g["ncl"], g["lb"]
    ncar = 2 * air_gen.NL // g["group"] - 1
    car = np.stack([sum(a[cb + m * ncl + l].astype(np.int64) << (lb * l) for l in range(ncl)) - g["coffset"] for m in range(ncar)])
    return sign, q, car


def positive_by_construction(g):
    """every product enters with a positive coefficient on vectors of positive coefficients: E = products - (values < p) is negative only
    where the products are smaller than those values (a slope below 2^128 in the curves' x3; never in Fq12's c11 = products - C), so no
    catalogue of honest records is asked for both signs there"""
    return all(coef > 0 and all(tm[0] > 0 for v in (va, vb) for tm in v[0]) for coef, va, vb in g["prods"])


REACHED_CARRY = {}


@pytest.mark.parametrize("kind", [0, 4, 1, 5, 2])
def test_catalogue_reaches_both_signs_zero_quotients_and_reports_its_carries(kind):
    t, air = trace_of(kind), air_of(kind)
    assert air.n_main == t.air.n_main and air.checked_base == t.air.checked_base
    exempt = [g["name"] for g in air.gadgets if positive_by_construction(g)]
    assert exempt == {0: ["x30"], 1: ["x31"], 2: ["c11"]}[kind % 4]
    worst = 0
    for g in air.gadgets:
        sign, q, car = gadget_cells(t, air, g)
        assert set(np.unique(sign).tolist()) <= {0, 1}
        if g["name"] not in exempt:
            assert sign.any() and not sign.all(), "gadget %s: the sign column is constant over the catalogue" % g["name"]
        assert (q == 0).all(axis=0).any(), "gadget %s: no row with all 17 quotient limbs zero" % g["name"]
        assert np.abs(car).max() < g["coffset"]
        worst = max(worst, int(np.abs(car).max()))
    REACHED_CARRY[kind] = worst
    print("kind %d: largest |carry| the catalogue reaches 2^%.2f (cells hold up to 2^%d)" % (kind, math.log2(worst), int(math.log2(air.gadgets[0]["coffset"]))))


def test_a_one_record_fq12_trace_has_constant_checked_columns():
    """the lookup columns' edge: a checked column that is ONE value over the whole trace (one histogram bin, T - 1 zero-count table
    values).  In the zero record's trace every checked column is (C, the quotients and the offset carries never move)"""
    recs = {r.name: r for r in E.records(2)}
    counts = {}
    for name in ("zero_zero_0", "pm1_pm1_max"):
        t = _oracle.Trace(2, arr(2, [recs[name]]))
        a = t.array()
        const = (a == a[:, :1]).all(axis=1)
        counts[name] = (int(const[t.air.checked_base: t.air.n_main].sum()), int(const.sum()))
        assert not failing_rows(t)
    print("constant (checked, all) columns of a one-record Fq12 trace, of (%d, %d):" % (t.air.n_checked, t.width), counts)
    assert counts["zero_zero_0"][0] == t.air.n_checked and counts["zero_zero_0"][1] >= 3000
    assert counts["pm1_pm1_max"][0] >= 1


@pytest.mark.parametrize("kind", [4, 5])
def test_hardened_inequality_witness_sits_at_limb_0_and_at_the_last_limb_with_either_sign(kind):
    recs = E.records(kind)
    t, air = trace_of(kind), air_of(kind)
    a = t.array()
    nc = 16 * (kind - 3)
    nz, px, rx = air.col("nz"), air.col("Px"), air.col("Rx")
    seen = set()
    for i, rec in enumerate(recs):
        if not rec.name.startswith("limb"):
            continue
        row = 512 * i                                       # R = offset, P = x, bit 0 set
        where = np.flatnonzero(a[nz: nz + nc, row])
        assert len(where) == 1, rec.name
        j = int(where[0])
        d = int(a[px + j, row]) - int(a[rx + j, row])
        assert d != 0 and int(a[nz + j, row]) * (d % GL) % GL == 1
        assert all(int(a[px + k, row]) == int(a[rx + k, row]) for k in range(nc) if k != j)       # the ONLY limb that differs
        seen.add((j, d > 0))
    assert seen == {(0, True), (0, False), (nc - 1, True), (nc - 1, False)}


# ---------------- the gadgets' bounds from the specification ----------------
def flag_value(a, idx, row):
    if idx < air_gen.N_PERIODIC:
        m, r0 = air_gen.PERIODICS[idx]
        return 1 if row % m == r0 else 0
    return sum(w for f, v, w in a.flagdefs[idx - air_gen.N_PERIODIC] if a.rowprog[row][f] == v)


def vec_interval(a, vec, fv):
    """[lo, hi] of any limb of a VEC: unchecked cells in [0, 2^16), checked cells in [0, 2^table_bits)"""
    lo = hi = 0
    for coef, base, _stride, flag, neg in vec[0]:
        f = coef
        if flag >= 0:
            f *= (1 - fv[flag]) if neg else fv[flag]
        m = f * ((1 << a.tbits) - 1 if base >= a.checked_base else 0xFFFF)
        lo, hi = lo + min(m, 0), hi + max(m, 0)
    return lo, hi


def gadget_flags(g):
    return sorted({tm[3] for _, va, vb in g["prods"] for v in (va, vb) for tm in v[0] if tm[3] >= 0} |
                  {tm[3] for _, va in g["lins"] for tm in va[0] if tm[3] >= 0})


def derive_e_bound(a, g):
    """max over the rows of the period and over k of |e_k|, e_k = sum coef (A * B)_k + sum coef A_k, by interval arithmetic; per k"""
    flags = gadget_flags(g)
    sigs = {}
    for row in range(1 << a.log_rows):
        sigs.setdefault(tuple(flag_value(a, f, row) for f in flags), row)
    best = [0] * 32
    worst_row = 0
    for sig, row in sigs.items():
        fv = dict(zip(flags, sig))
        lo, hi = [0] * 32, [0] * 32
        for coef, va, vb in g["prods"]:
            (alo, ahi), (blo, bhi) = vec_interval(a, va, fv), vec_interval(a, vb, fv)
            c = [alo * blo, alo * bhi, ahi * blo, ahi * bhi]
            plo, phi = sorted((coef * min(c), coef * max(c)))
            for k in range(va[1] + vb[1] - 1):
                cnt = min(k, va[1] - 1) - max(0, k - vb[1] + 1) + 1
                lo[k] += cnt * plo
                hi[k] += cnt * phi
        for coef, va in g["lins"]:
            l, h = sorted(coef * x for x in vec_interval(a, va, fv))
            for k in range(va[1]):
                lo[k] += l
                hi[k] += h
        e = [max(-lo[k], hi[k]) for k in range(32)]
        if max(e) > max(best):
            worst_row = row
        best = [max(x, y) for x, y in zip(best, e)]
    return best, worst_row


def derive_carry_bound(g, e):
    """the largest |c_m| an honest row can need, from |d_k| <= |e_k| + (q p)_k with every quotient limb at 0xFFFF:
    c_m = (c_{m-1} - D_m) / 2^(16 g), D_m = sum_t 2^(16 t) d_{g m + t};  also the largest |D_m|"""
    grp = g["group"]
    qp = [0xFFFF * sum(air_gen.P_LIMBS[k - i] for i in range(air_gen.NQ) if 0 <= k - i < air_gen.NL) for k in range(32)]
    d = [e[k] + qp[k] for k in range(32)]
    c, cmax, dmax = 0, 0, 0
    for m in range(32 // grp - 1):
        D = sum(d[grp * m + t] << (16 * t) for t in range(grp))
        c = (c + D) >> (16 * grp)
        cmax, dmax = max(cmax, c), max(dmax, D)
    return cmax, dmax


EXPECTED_LOG2_E = {"g1": 37.58, "g1h": 37.58, "g2": 38.58, "g2h": 38.58, "fq12": 42.60, "mapg2": 39.00, "pairing": 42.60}


@functools.lru_cache(None)
def all_airs():
    out = []
    for mode in ("u16", "u8"):
        out += [air_gen.build_curve("g1", mode, 1), air_gen.build_curve("g2", mode, 2), air_gen.build_fq12(mode), air_gen.build_map_g2(mode),
                air_gen.build_curve("g1", mode, 1, hardened=True), air_gen.build_curve("g2", mode, 2, hardened=True), air_gen.build_pairing(mode)]
    return out


@pytest.mark.parametrize("idx", range(14), ids=lambda i: "%s_%s" % (("g1", "g2", "fq12", "mapg2", "g1h", "g2h", "pairing")[i % 7], ("u16", "u8")[i // 7]))
def test_declared_gadget_bounds_hold_by_interval_arithmetic_over_the_program(idx):
    """for every gadget: the derived worst |e_k| is within 2^bound_bits; the carries it implies (the q p term included) fit the carry
    cells; the generator's soundness inequality |D_m - c_{m-1} + 2^(16 g) c_m| < the Goldilocks prime holds with the DERIVED bound, and in
    the sharper form that takes every cell at its range's end"""
    a = all_airs()[idx]
    worst_e, worst_at = 0, None
    for g in a.gadgets:
        e, row = derive_e_bound(a, g)
        emax = max(e)
        assert emax <= 1 << g["bound_bits"], "%s gadget %s row %d: |e_k| can reach 2^%.2f > 2^%d" % (a.name, g["name"], row, math.log2(emax), g["bound_bits"])
        cmax, dmax = derive_carry_bound(g, e)
        ncl, lb, grp = g["ncl"], g["lb"], g["group"]
        assert g["coffset"] == 1 << (ncl * lb - 1)
        assert cmax <= g["coffset"] - 1, "%s gadget %s: a carry can reach 2^%.2f, its cells hold 2^%d" % (a.name, g["name"], math.log2(cmax), ncl * lb - 1)
        # tools/air_gen.py Air.gadget `worst`, with the derived bound in the place of 2^bound_bits
        worst = (1 << (ncl * lb - 1 + 16 * grp)) + (emax << (16 * (grp - 1) + 1)) + (1 << (ncl * lb))
        assert worst < (1 << 64) - (1 << 32)
        # every range-checked assignment: |c| <= 2^(ncl lb - 1), |D_m| <= dmax (d_k with q p at its largest)
        assert (g["coffset"] << (16 * grp)) + dmax + g["coffset"] < GL
        if emax > worst_e:
            worst_e, worst_at = emax, (g["name"], row, cmax)
    print("%s_%s: derived max |e_k| = 2^%.2f (gadget %s, row %d of the period), declared 2^%d; derived max |carry| 2^%.2f, cells hold 2^%d" % (
        a.name, a.mode, math.log2(worst_e), worst_at[0], worst_at[1], a.gadgets[0]["bound_bits"], math.log2(worst_at[2]),
        a.gadgets[0]["ncl"] * a.gadgets[0]["lb"] - 1))
    assert abs(math.log2(worst_e) - EXPECTED_LOG2_E[a.name]) < 0.01


# ---------------- the committed tables ----------------
def test_air_tables_header_is_what_the_generator_writes(tmp_path, monkeypatch):
    (tmp_path / "data").mkdir()
    monkeypatch.setattr(air_gen, "ROOT", str(tmp_path))
    air_gen.main()
    new = (tmp_path / "data" / "air_tables.h").read_bytes()
    assert new == open(os.path.join(ROOT, "data", "air_tables.h"), "rb").read(), "data/air_tables.h is stale: run tools/air_gen.py"
