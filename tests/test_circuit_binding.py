"""Every outer circuit scanned for witness cells that no constraint binds (tests/_binding_scan.py; CPU): the counterpart, for the PLONK
statement circuits on CircuitBuilder, of tests/test_oracle_soundness.py::test_every_main_column_is_constrained_on_some_row.

The catalogue is every circuit at the smallest case its own test module builds, through that module's build / witness / honest helpers:
MerkleOpeningCircuit (the `opening` fixture's case), FriFoldCircuit, FriInitialCircuit (K = 2), FriQueryRoundCircuit and FriProofCircuit
at ROUND_A16, PlonkVanishingCircuit at every name of tests/_plonk_vanishing_cases.py and every variant of
tests/test_plonk_vanishing_mds.py (with and without poseidon_mds), PlonkVerifierCircuit at every CASES key, SippTranscriptCircuit(4),
and the test circuits BasicCircuit (`inner-basic`, and `inner-ragged` under one selector column), ManyGenerators (16 generators),
RangeCheckCircuit, XorLookupCircuit and BlindCircuit with and without lookups.

Asserted per circuit: the honest witness satisfies every row; the SILENT classes of the class scan are exactly the cells the rules of
CLASS_RULES name, no class is UNDEFINED; the silent pairs of the re-split scan are exactly the pairs PAIR_RULES excuse, each under every
move or under none.  A rule is a predicate with its reason and a circuit in which it must match, so that none goes stale.  The
transcript's exception is exactly 112 cells (wires 5 and 43 of 56 U32Arithmetic rows, lo = 0 on every one).  A silent cell without a
rule is a constraint missing in a builder: none was found.

ManyGenerators is no statement -- only witness generation runs it: a BaseSplit row fed a wide value is not satisfied by its own
generator's output (20 rows of the table of seed 7) and the plain Poseidon family has no program.  Its unsatisfied rows are never asked
and the classes that touch them (59) are not scanned; the rest is scanned like every other circuit.

Planted holes: LeSum32 without its sum constraint is reported by the class scan (as undefined: the sum cell is wired into the reduce
row and onto the column sums of q m + rem, which still object; `silent` is what an output nobody consumes would be); BaseSplit64
without one limb's booleanity constraint, and U32Range without one limb's range constraint,
are reported by the re-split scan and by it alone.

CPU time as measured (one process, the module alone, 628 s for its 81 tests; a circuit is built once):
  class scan    verifier-* 24 - 27 s (102 - 123 k classes at 2^11 and 2^13 rows), merkle 12 s (48 k), transcript-n4 10 s (36 k),
                vanishing-* 8 - 10 s (15 - 31 k), fri_proof 4.6 s, fri_query_round 4.2 s, fri_fold 3.3 s, every other below 1 s
  re-split scan verifier-* 20 - 21 s (78 - 82 k pairs), fri_proof 19 s, fri_query_round 16 s, many-generators-16 14 s, fri_fold 14 s,
                transcript-n4 14 s, vanishing-* 12 s, blind* 12 s, merkle 11 s, fri_initial 11 s, xor_lookup 10 s (in each about 10 s are
                the one PoseidonSwap row: 135 read wires, 18 k pairs), the three small circuits below 0.1 s
Every row is judged by a description that keeps only its own gate (the other gates' filters vanish on it), which is five times faster
than evaluating every gate's program on every row; no re-split scan comes near the minute at which the rows per gate would be cut."""
import collections
import functools

import numpy as np
import pytest

from sipp_amd import circuit as ci
from sipp_amd.fri_initial import reducing_layout
from tests import _binding_scan as bs
from tests import _oracle

P = _oracle.P


# ---- the catalogue: every outer circuit at the smallest case its own test module builds --------------------------------------------------
def _from(module, key, name, args_of=lambda b: b["args"]):
    """a circuit built and replayed by its test module's own build() / witness()"""
    b = module.build(key)
    w, pis, pih = module.witness(b)
    c = b["c"]
    return bs.Subject(name, c, b["cs"], c.partial_witness(*args_of(b)), pih, honest=w)


def _merkle():
    """tests/test_merkle_circuit.py builds its case in a fixture: the fixture's function is called as the module's tests get it"""
    from tests import test_merkle_circuit as tm
    o = getattr(tm.opening, "__wrapped__", None) or tm.opening._get_wrapped_function()
    o = o()
    w, pis, pih = tm.witness(o)
    return bs.Subject("merkle", o["mc"], o["cs"], o["mc"].partial_witness(o["cap"], o["idx"], o["leaves"], o["sib"]), pih, honest=w)


def _fri_fold():
    from tests import test_fri_fold_circuit as tf
    from tests.test_fri_verifier_circuit import ROUND_A16
    return _from(tf, ROUND_A16, "fri_fold", lambda b: (b["betas"], b["final"], b["queries"]))


def _fri_initial():
    from tests import test_fri_initial_circuit as ti
    from tests.test_fri_verifier_circuit import ROUND_A16
    o = ti.build(ROUND_A16, (2, 2))
    w, pis, pih = ti.witness(o)
    return bs.Subject("fri_initial", o["c"], o["cs"], o["c"].partial_witness(*o["args"]), pih, honest=w)


def _fri_round():
    from tests import test_fri_verifier_circuit as tv
    return _from(tv, tv.ROUND_A16, "fri_query_round")


def _fri_proof():
    from tests import test_fri_proof_circuit as tp
    return _from(tp, tp.ROUND_A16, "fri_proof")


def _vanishing(name):
    from tests import test_plonk_vanishing_circuit as tv
    return _from(tv, name, "vanishing-" + name)


def _vanishing_mds(variant):
    from tests import test_plonk_vanishing_mds as tm
    return _from(tm, variant, "vanishing-mds-" + variant)


def _verifier(case):
    from tests import test_plonk_verifier_circuit as tj
    return _from(tj, case, "verifier-" + case)


def _transcript():
    from tests import test_transcript_circuit as tt
    b = tt.honest(4)
    c = b["c"]
    return bs.Subject("transcript-n4", c, b["cs"], c.partial_witness(b["st"], b["rw"], b["ch"]), b["pih"], honest=b["w"])


def _inner(name):
    """BasicCircuit under two selector columns (`basic`) and under one (`ragged`), as tests/_plonk_vanishing_cases.py replays them"""
    from tests import _plonk_vanishing_cases as cases
    o = cases.inner(name)
    pih = _oracle.hash_no_pad(np.array(o["pis"], dtype=np.uint64))
    return bs.Subject("inner-" + name, o["c"], o["cs"], o["pw"], pih, honest=o["w"])


def _many_generators():
    """tests/_many_generators.py at sixteen generators.  Only witness generation runs these circuits: the plain Poseidon family has no
    program and a BaseSplit row fed a wide value is not satisfied, so the scan is of the classes whose rows the replayed table satisfies"""
    from tests import _many_generators as mg
    c = mg.ManyGenerators(*mg.CIRCUITS["16"])
    table, consts = c.table(7)
    s = bs.Subject("many-generators-16", c, c.constants_sigmas(), table, [0, 0, 0, 0], written=np.zeros(table.shape, dtype=bool))
    s.written_override = s.honest != table                     # a random table: what the replay changed is what was written
    s.mute = set(s.unsatisfied_rows())
    return s


def _test_circuit(c, args):
    pis = c.public_inputs(*args[:c.n_public_args])
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    with bs.readings_for_test_circuits():
        return bs.Subject(type(c).__name__, c, c.constants_sigmas(), c.partial_witness(*args), pih)


def _range_check():
    from tests._lookup_circuit import RangeCheckCircuit
    from tests.test_lookup_builder import VALUES
    return _test_circuit(RangeCheckCircuit(n_values=len(VALUES), bits=5), (VALUES,))


def _xor_lookup():
    from tests._lookup_tables_circuit import XorLookupCircuit
    return _test_circuit(XorLookupCircuit(), (5, 9, 12))


def _blind(lookups):
    from tests import _blinding_cases as bc
    c = bc.circuit(lookups)
    return _test_circuit(c, (c.value(9, 12), 9, 12))


def _names(module, attr):
    import importlib
    return sorted(getattr(importlib.import_module(module), attr))


SUBJECTS = {"merkle": _merkle, "fri_fold": _fri_fold, "fri_initial": _fri_initial, "fri_query_round": _fri_round, "fri_proof": _fri_proof,
            "transcript-n4": _transcript, "inner-basic": lambda: _inner("basic"), "inner-ragged": lambda: _inner("ragged"),
            "many-generators-16": _many_generators, "range_check": _range_check, "xor_lookup": _xor_lookup,
            "blind": lambda: _blind(False), "blind-lookups": lambda: _blind(True)}
SUBJECTS.update({"vanishing-" + k: functools.partial(_vanishing, k) for k in _names("tests._plonk_vanishing_cases", "NAMES")})
SUBJECTS.update({"vanishing-mds-" + k: functools.partial(_vanishing_mds, k) for k in _names("tests.test_plonk_vanishing_mds", "VARIANTS")})
SUBJECTS.update({"verifier-" + k: functools.partial(_verifier, k) for k in _names("tests.test_plonk_verifier_circuit", "CASES")})


@functools.lru_cache(maxsize=None)
def subject(name):
    return SUBJECTS[name]()


@functools.lru_cache(maxsize=None)
def class_scan(name):
    with bs.readings_for_test_circuits():
        return bs.class_scan(subject(name))


@functools.lru_cache(maxsize=None)
def resplit_scan(name):
    return bs.resplit_scan(subject(name))


# ---- the exception rules: a predicate with its reason, and a circuit in which it must match ---------------------------------------------
def _generator(s, r):
    """the generator of the gate row r holds, or None"""
    return next((g for g in s.c.generators() if g[2] == int(s.gate[r])), None)


def _u32_inverse_when_lo_is_zero(s, x):
    r, w = x % s.n, x // s.n
    g = _generator(s, r)
    if g is None or g[0] != ci.GEN_U32_ARITHMETIC:
        return False
    op, t = divmod(w, g[4])
    return op < g[3] and t == 5 and int(s.honest[g[4] * op + 3, r]) == 0


def _blinding_row_cells(s, x):
    rows = s.c.blind_rows
    return x % s.n in set(rows["regular"]) | {r for pair in rows["pairs"] for r in pair}


# name -> (reason, predicate(subject, flat cell), the catalogue circuit in which it must match a silent cell)
CLASS_RULES = {
    "u32_inverse_when_lo_is_zero": (
        "U32Arithmetic says (inverse (2^32 - 1 - hi) - 1) lo = 0: where lo = 0 it holds whatever the inverse cell holds, and nothing reads "
        "the cell; the split is canonical there anyway (lo = 0)", _u32_inverse_when_lo_is_zero, "transcript-n4"),
    "blinding_row_cells": (
        "blinding rows and the routed pairs that randomise Z are free by design: their gate has no constraints",
        _blinding_row_cells, "blind"),
}


def _dead_wires(s, r):
    """{wire: (rule, product)} of row r: the wires whose value the row's constraints cannot see because a zero stands beside them.
    product: (op, operand) where two such wires are the factors of ONE product -- moved together they make it non-zero -- else None"""
    g, row, k = _generator(s, r), [int(v) for v in s.honest[:, r]], s.consts
    out = {}
    if g is None:
        return out
    kind, p = g[0], g[3:8]
    if kind == ci.GEN_RANDOM_ACCESS:
        copies, stride, bits = p[:3]
        for cp in range(copies):
            b = stride * cp
            out.update({b + 2 + t: ("random_access_unselected_item", None) for t in range(1 << bits) if t != row[b]})
    elif kind in (ci.GEN_ARITHMETIC_EXT, ci.GEN_QUOTIENT_EXT):
        c0, c1 = int(k[p[1], r]) % P, int(k[p[2], r]) % P
        for op in range(p[0]):
            b = 8 * op
            a, m = (row[b], row[b + 1]), (row[b + 2], row[b + 3])
            if c0 == 0 or m == (0, 0):
                out.update({b + l: ("ext_product_operand_beside_zero", (op, "a") if c0 else None) for l in range(2)})
            if c0 == 0 or a == (0, 0):
                out.update({b + 2 + l: ("ext_product_operand_beside_zero", (op, "m") if c0 else None) for l in range(2)})
            if c1 == 0:
                out.update({b + 4 + l: ("ext_product_operand_beside_zero", None) for l in range(2)})
    elif kind in (ci.GEN_REDUCING, ci.GEN_REDUCING_EXT):
        lay = reducing_layout(p[0], kind == ci.GEN_REDUCING_EXT)
        multiplied = [lay["old"], lay["old"] + 1] + list(range(lay["accs"], lay["accs"] + 2 * (p[0] - 1)))
        if not any(row[w] for w in multiplied):
            out.update({0: ("reducing_alpha_beside_zero_accumulators", None), 1: ("reducing_alpha_beside_zero_accumulators", None)})
    return out


def pair_rule(dead, i, j):
    """the rule that excuses the ordered pair (i, j) of a row whose dead wires are `dead`, or None"""
    if i not in dead or j not in dead:
        return None
    (rule, pi), (_, pj) = dead[i], dead[j]
    if pi is not None and pj is not None and pi[0] == pj[0] and pi[1] != pj[1]:
        return None                                             # both factors of one product: a' m' != 0
    return rule


# name -> (reason, the catalogue circuit in which it must match a silent pair); the predicate is _dead_wires / pair_rule
PAIR_RULES = {
    "random_access_unselected_item": (
        "RandomAccess multiplies every item but items[index] by a zero selector product: the row cannot see the others, the rows they are "
        "copied from bind them", "inner-basic"),
    "ext_product_operand_beside_zero": (
        "out = c0 a m + c1 c over the extension: an addend under c1 = 0, a factor beside a zero factor (or c0 = 0), every operand of a short "
        "row's unused ops (all zero).  Two factors of ONE product are not excused together", "vanishing-basic"),
    "reducing_alpha_beside_zero_accumulators": (
        "acc_i = acc_(i-1) alpha + c_i: on a row whose old accumulator and every accumulator alpha multiplies are zero (a chain's first "
        "row behind a zero) alpha meets only zeros", "fri_initial"),
}


# ---- the scans over the catalogue -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SUBJECTS))
def test_the_honest_witness_satisfies_every_row(name):
    s = subject(name)
    assert sorted(s.mute) == s.unsatisfied_rows()               # no row but the synthetic circuit's, which are known and never asked
    assert bool(s.mute) == (name == "many-generators-16")


@pytest.mark.parametrize("name", sorted(SUBJECTS))
def test_the_silent_classes_are_the_named_exceptions(name):
    s, out = subject(name), class_scan(name)
    print("%s: %d classes in %.1f s, %d silent, %d undefined, %d skipped" % (name, out["classes"], out["seconds"], len(out["silent"]),
                                                                           len(out["undefined"]), out["skipped"]))
    assert out["classes"] >= 16
    assert out["undefined"] == [], [unflat(s, cls) for cls in out["undefined"][:5]]
    silent = {x for cls in out["silent"] for x in cls}
    matched = {int(x): [n for n, (_, pred, _) in CLASS_RULES.items() if pred(s, int(x))] for x in np.flatnonzero(out["scanned"])}
    matched = {x: names for x, names in matched.items() if names}
    assert sorted(silent - set(matched)) == [], "silent cells without a reason: a constraint is missing in the builder"
    assert sorted(set(matched) - silent) == [], "cells a rule excuses are bound: the rule is stale"


def unflat(s, cls):
    return [(s.c.gate_names[int(s.gate[x % s.n])], int(x // s.n), int(x % s.n)) for x in cls]


@pytest.mark.parametrize("name", sorted(SUBJECTS))
def test_the_silent_resplit_pairs_are_the_named_exceptions(name):
    s, rs = subject(name), resplit_scan(name)
    print("%s: %d pairs in %.1f s, %d silent mutations" % (name, rs["pairs"], rs["seconds"], len(rs["silent"])))
    times = collections.Counter((g, r, i, j) for g, r, i, j, B, sign in rs["silent"])
    expected = set()
    for g, rows in bs.resplit_rows(s).items():
        reads = bs.read_wires(s.circ, g)
        per_pair = 2 * (2 if len(reads) > bs.WIDE_GATE else len(bs.RESPLIT_B))
        for r in rows:
            dead = _dead_wires(s, r)
            expected |= {(g, r, i, j) for i in reads for j in reads if i != j and pair_rule(dead, i, j)}
            assert all(v == per_pair for (gg, rr, _, _), v in times.items() if (gg, rr) == (g, r)), "a pair silent under some moves only"
    assert sorted(set(times) - expected)[:8] == [], "silent pairs without a reason: a range or booleanity constraint is missing"
    assert sorted(expected - set(times))[:8] == [], "pairs a rule excuses are seen by the row: the rule is stale"


def test_the_transcripts_exception_is_the_112_inverse_cells_all_beside_a_zero_lo():
    s, out = subject("transcript-n4"), class_scan("transcript-n4")
    cells = sorted(x for cls in out["silent"] for x in cls)
    assert len(cells) == 112 and all(len(cls) == 1 for cls in out["silent"])
    rows = sorted({x % s.n for x in cells})
    assert len(rows) == 56 and set(rows) <= set(s.c.u32_rows["arith"])
    assert sorted({x // s.n for x in cells}) == [5, 43] and all((5 * s.n + r in cells) and (43 * s.n + r in cells) for r in rows)
    assert all(int(s.honest[x // s.n - 2, x % s.n]) == 0 for x in cells)        # lo, two wires in front of the inverse cell
    # and on every other op of every U32Arithmetic row lo != 0: there the inverse cell is bound
    others = [(w, r) for r in s.c.u32_rows["arith"] for w in (5, 43) if w * s.n + r not in cells]
    assert others and all(int(s.honest[w - 2, r]) != 0 for w, r in others)


def test_every_rule_has_a_reason_and_matches_where_it_says():
    for name, (reason, pred, where) in CLASS_RULES.items():
        s, out = subject(where), class_scan(where)
        assert len(reason) > 20 and any(pred(s, x) for cls in out["silent"] for x in cls), name
    for name, (reason, where) in PAIR_RULES.items():
        s, rs = subject(where), resplit_scan(where)
        assert len(reason) > 20 and where in SUBJECTS
        assert any(pair_rule(_dead_wires(s, r), i, j) == name for g, r, i, j, B, sign in rs["silent"]), name


# ---- planted holes: the scans notice a real defect ----------------------------------------------------------------------------------------
def _holed(name, gate, which):
    s = subject(name)
    return bs.Subject(name + "-holed", s.c, s.consts, s.partial, s.pih, honest=s.honest,
                      circ=bs.drop_constraint(s.c.circuit(), gate, which))


def test_drop_constraint_takes_one_constraint_out_and_keeps_the_rest():
    from tests import _merkle_reading as mr
    circ = subject("transcript-n4").c.circuit()
    gate = circ["gate_names"].index("LeSum32")
    holed = bs.drop_constraint(circ, gate, 0)
    for g, (a, b) in enumerate(zip(circ["gates"], holed["gates"])):
        was, now = mr.decode(circ["programs"], a[4], a[5]), mr.decode(holed["programs"], b[4], b[5])
        assert tuple(a[:4]) == tuple(b[:4]) and now == (was[1:] if g == gate else was)
    assert len(holed["programs"]) < len(circ["programs"])
    import ctypes as C
    check = _oracle._plonk_gates_lib().orc_plonk_circuit_check
    assert check(C.byref(_oracle.plonk_circuit(holed)), C.byref(_oracle.plonk_params(80, 8, 2))) == 0          # still a well-formed description


def test_a_dropped_sum_constraint_is_reported_by_the_class_scan():
    """LeSum32 without its first constraint (sum of the limbs - wire 0).  The sum cell is wired on -- into the NonnativeReduce row and
    onto the column sums of q m + rem -- so the consumers still object when its class is moved: it is reported as UNDEFINED (the row
    whose generator writes it does not object), which on the honest circuit no class is.  A sum cell nobody consumed would be silent."""
    from sipp_amd.transcript import LE_SUM32
    c = subject("transcript-n4").c
    row = int(np.flatnonzero(c.gate == LE_SUM32)[3])
    holed = _holed("transcript-n4", LE_SUM32, 0)
    out = bs.class_scan(holed, only_rows=[row])
    reported = out["silent"] + out["undefined"]
    assert [cls for cls in reported if 0 * c.n + row in cls] and all(0 * c.n + row in cls for cls in reported)
    assert out["classes"] == 33                                 # the sum and its 32 limbs
    honest = bs.class_scan(subject("transcript-n4"), only_rows=[row])
    assert honest["silent"] == honest["undefined"] == [] and honest["classes"] == 33


@pytest.mark.parametrize("gate_name,limb", [("BaseSplit64", 5), ("U32Range", 7)])
def test_a_dropped_booleanity_or_range_constraint_is_reported_by_the_resplit_scan_alone(gate_name, limb):
    """constraint 1 + limb of a split gate is the limb's range constraint (x (x - 1), or x (x - 1) (x - 2) (x - 3) for a 2-bit limb): without
    it the row accepts limb + B beside a neighbour - 1 where B is the neighbour's weight over the limb's.  No one-cell move shows that:
    the class scan of the row's cells finds nothing"""
    c = subject("transcript-n4").c
    gate = c.gate_names.index(gate_name)
    holed = _holed("transcript-n4", gate, 1 + limb)
    rows = bs.resplit_rows(holed)[gate]
    rs = bs.resplit_scan(holed, only_rows=rows)
    assert rs["silent"] and all(g == gate and r in rows for g, r, i, j, B, sign in rs["silent"])
    assert {1 + limb} <= {i for g, r, i, j, B, sign in rs["silent"]} | {j for g, r, i, j, B, sign in rs["silent"]}
    assert all(1 + limb in (i, j) for g, r, i, j, B, sign in rs["silent"])
    out = bs.class_scan(holed, only_rows=rows)
    assert out["silent"] == out["undefined"] == [] and out["classes"] > len(rows)
    assert bs.resplit_scan(subject("transcript-n4"), only_rows=rows)["silent"] == []
