"""The binding scan's witnesses through the device prover (tests/_binding_scan.py, tests/test_circuit_binding.py): one smallest case per
circuit family -- 2^10 or 2^11 rows, PlonkParams(80, 8, 2) and the outer FRI parameters every family's own GPU test proves under.  Per
family, chosen by a fixed seed among what the CPU scan judges:

  generated      a class that holds a generator-written cell and is bound: all its cells moved by one
  input          a bound class of a witness input (not a public input), where the circuit has witness inputs
  resplit        on a BaseSplit row, limb l + 2^bits beside limb l + 1 - 1: the sum holds, only the limb's range constraint objects
  <rule>         one class of every exception rule of tests/test_circuit_binding.CLASS_RULES that the circuit has a cell of

For every mutated table W' the RAW entry ctx.plonk_prove_gates(dev(W'), ...), which does not regenerate the witness, must give
_oracle.plonk_prove_gates(W', ...) word for word: a bound mutation makes a "quotient" that is no polynomial of the degree the prover
assumes, and the device's coset iNTT must alias exactly as the oracle's does.  The library's verifier and the oracle's must then both
refuse a bound mutation at the same stage (a == -b, whatever the stage) and both accept an exception cell; afterwards the same ctx
proves the honest table and both accept.

Left out: RangeCheckCircuit and XorLookupCircuit (the oracle has no prover for the lookup argument to compare with) and ManyGenerators
(no statement: its random table leaves rows unsatisfied).  BlindCircuit is proved here WITHOUT hiding: its blinding rows are ordinary
rows of a gate without constraints."""
import functools

import numpy as np
import pytest

from sipp_amd import circuit as ci
from tests import _binding_scan as bs
from tests import _oracle, _verify
from tests._device import dev
from tests.test_circuit_binding import CLASS_RULES, subject
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

P = _oracle.P
DIGEST = (97, 98, 99, 100)
SEED = 20262
# family -> the kinds it has: the Merkle, fold and initial circuits take everything from public inputs, the vanishing circuits also
# have no split row; only the transcript has u32 arithmetic rows, only `blind` blinding rows (and no split row)
CASES = {"merkle": ("generated", "resplit"), "fri_fold": ("generated", "resplit"), "fri_initial": ("generated", "resplit"),
         "fri_query_round": ("generated", "input", "resplit"), "fri_proof": ("generated", "input", "resplit"),
         "vanishing-basic": ("generated",), "vanishing-mds-poseidon_route": ("generated",),
         "verifier-basic": ("generated", "input", "resplit"),
         "transcript-n4": ("generated", "input", "resplit", "u32_inverse_when_lo_is_zero"),
         "inner-basic": ("generated", "input", "resplit"), "blind": ("generated", "input", "blinding_row_cells")}
FAMILIES = tuple(CASES)
KINDS = ("generated", "input", "resplit") + tuple(sorted(CLASS_RULES))


@functools.lru_cache(maxsize=None)
def mutations(name):
    """{kind: (bound?, the mutated table)} of one family, from the CPU scan's judge under a fixed seed"""
    s = subject(name)
    c, n = s.c, s.n
    rng = np.random.default_rng(SEED)
    honest, partial = s.honest.reshape(-1), s.partial.reshape(-1)
    copied = np.zeros(len(honest), dtype=bool)
    copied[c.schedule()["copy_dst"].astype(np.int64)] = True
    generated = (honest != partial) & ~copied                   # certainly a generator's: changed by the replay, nobody's copy
    cycle_of = {x: k for k, cyc in enumerate(c.cycles) for x in cyc}
    cls_of = lambda x: np.asarray(c.cycles[cycle_of[x]] if x in cycle_of else [x], dtype=np.int64)

    def moved(cls):
        w = s.honest.copy()
        w.reshape(-1)[cls] = np.uint64((int(honest[cls[0]]) + 1) % P)
        return w

    out = {}
    with bs.readings_for_test_circuits():
        cells = np.flatnonzero(generated & s.constrained[np.arange(len(honest)) % n])
        for x in rng.permutation(cells)[:64]:
            if bs.judge(s, cls_of(int(x)), generated) == "bound":
                out["generated"] = (True, moved(cls_of(int(x))))
                break
        for k in rng.permutation(len(c.in_cycle))[:64]:
            cls = np.asarray(c.in_cycle[k], dtype=np.int64)
            if bs.judge(s, cls, generated) == "bound":
                out["input"] = (True, moved(cls))
                break
        for rule, (_, pred, _) in sorted(CLASS_RULES.items()):
            hit = [int(x) for x in rng.permutation(np.flatnonzero(generated)) if pred(s, int(x))][:1]
            if hit:
                assert bs.judge(s, cls_of(hit[0]), generated) == "silent"
                out[rule] = (False, moved(cls_of(hit[0])))
    splits = [(g[2], g[3], g[4]) for g in c.generators() if g[0] == ci.GEN_BASE_SPLIT and g[3] >= 2]
    rows = [(int(r), limbs, bits) for gate, limbs, bits in splits for r in np.flatnonzero(s.gate == gate)]
    if rows:
        r, limbs, bits = rows[int(rng.integers(len(rows)))]
        l = int(rng.integers(limbs - 1))
        w = s.honest.copy()
        w[1 + l, r] = (int(w[1 + l, r]) + (1 << bits)) % P
        w[2 + l, r] = (int(w[2 + l, r]) - 1) % P
        assert s.rows.nonzero(np.ascontiguousarray(w[:, r]), r)
        out["resplit"] = (True, w)
    assert "generated" in out
    return out


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)                   # the raw entry commits constants_sigmas itself: tests/test_gpu_plonk.py's size
    yield c
    c.close()


@pytest.fixture(scope="module")
def family(ctx, request):
    """per family: the subject, the device constants_sigmas, the oracle-side parameters, the raw prove call"""
    import sipp_amd
    s = subject(request.param)
    c = s.c
    cs = c.constants_sigmas()
    circ = c.circuit()
    ofp = fri(c.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp, gp, gc = to_params(ofp), sipp_amd.PlonkParams(80, 8, 2), sipp_amd.PlonkCircuit.from_dict(circ)
    flat = s.honest.reshape(-1)
    pis = [int(flat[x]) for x in c.pi_cells]
    assert [int(v) for v in _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))] == s.pih
    o = {"name": request.param, "s": s, "cs": cs, "circ": circ, "ofp": ofp, "op": _oracle.plonk_params(80, 8, 2), "pis": pis, "ctx": ctx,
         "d_cs": dev(cs), "prove": lambda w: ctx.plonk_prove_gates(dev(w), o["d_cs"], c.log_n, gp, gfp, gc, DIGEST, pis),
         "cap": _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=4).cap}
    return o


def oracle_proof(o, w):
    return _oracle.plonk_prove_gates(w, o["cs"], o["s"].c.log_n, o["op"], o["ofp"], o["circ"], DIGEST, o["pis"])


def verdicts(o, pf):
    """(the library's refusing stage, the oracle's status): 0 and 0, or a stage and its negative"""
    return (_verify.lib_plonk_verify(pf, o["cap"], o["op"], o["ofp"], o["circ"], DIGEST),
            _oracle.plonk_verify_gates(pf, o["cap"], o["op"], o["ofp"], o["circ"], DIGEST))


def same_words(got, want):
    assert len(got) == len(want)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "first mismatch at word %d of %d" % (diff[0], len(want))


@pytest.mark.parametrize("family,kind", [(f, k) for f in FAMILIES for k in CASES[f]], indirect=["family"])
def test_a_mutated_table_is_proved_as_the_oracle_proves_it_and_judged_alike(family, kind):
    o = family
    muts = mutations(o["name"])
    assert sorted(muts) == sorted(CASES[o["name"]])
    bound, w = muts[kind]
    assert (w != o["s"].honest).any()
    pf = o["prove"](w)
    same_words(pf, oracle_proof(o, w))
    a, b = verdicts(o, pf)
    assert a == -b, "the verifiers disagree: library stage %d, oracle %d" % (a, b)
    assert (a != 0) == bound, (kind, a, b)
    # the same ctx proves the honest table afterwards, and both accept
    if "honest" not in o:
        o["honest"] = oracle_proof(o, o["s"].honest)
    good = o["prove"](o["s"].honest)
    same_words(good, o["honest"])
    assert verdicts(o, good) == (0, 0)


def test_every_kind_is_reached_by_some_family():
    assert {k for kinds in CASES.values() for k in kinds} == set(KINDS)
