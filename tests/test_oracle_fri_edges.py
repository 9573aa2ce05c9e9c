"""The case table of tests/_fri_cases.py on the CPU: every case is proved by oracle/fri.c and accepted by the oracle's verifier, by the
library's host verifier (sipp_fri_verify_openings) and, up to 2^11 coefficients, by the independent Python reading
(oracle/py/plonky2_generic.py) query by query.  This keeps the table that tests/test_gpu_fri_edges.py compares the device against honest
without a GPU, and holds the library's verifier to the same edges: the point zero, points with a zero component, batches without a
polynomial, no reduction round, caps as high as a layer, 1 and 1024 queries, a challenger that arrives with pending input or output."""
import numpy as np
import pytest

from oracle.py import plonky2_generic as g2
from tests import _fri_cases as fc
from tests import _oracle, _verify


def python_reading_accepts(inst, pf):
    """replay the flat proof with the Python reading: transcript, proof of work, every Merkle path, every query's folds"""
    case, fp, log_n = inst.case, inst.fp, inst.log_n
    pf = [int(x) for x in pf]
    arities = [fp.arity_bits[i] for i in range(fp.n_rounds)]
    log_m = log_n + fp.rate_bits
    pos = [8]

    def take(k):
        v = pf[pos[0]:pos[0] + k]
        assert len(v) == k
        pos[0] += k
        return v
    ch = g2.Challenger()
    ch.observe_many([case.stress_seed, 1, 2] if case.stress_seed is not None else list(case.prefix))
    for _ in range(case.gets):
        ch.get()
    opened = []
    for pt, ranges in inst.batches:
        vals = [g2.Ext(*take(2)) for _ in range(sum(e - b for _, b, e in ranges))]
        for v in vals:
            ch.observe_ext(v)
        opened.append(vals)
    alpha = ch.get_ext()
    caps, betas = [], []
    for _ in arities:
        caps.append([take(4) for _ in range(1 << fp.cap_height)])
        ch.observe_cap(caps[-1])
        betas.append(ch.get_ext())
    final_poly = [g2.Ext(*take(2)) for _ in range((1 << log_n) >> sum(arities))]
    for c in final_poly:
        ch.observe_ext(c)
    assert g2.pow_ok(g2.pow_response(ch, fp.pow_rule, take(1)[0]), fp.pow_bits)
    for _ in range(fp.num_queries):
        x = ch.get() % (1 << log_m)
        rows = []
        for o in inst.oracles:
            row, sib = take(o.ncols + o.n_salt), [take(4) for _ in range(log_m - fp.cap_height)]
            assert g2.verify_merkle_proof_to_cap(row, x, [[int(v) for v in d] for d in o.cap], sib)
            rows.append(row)
        steps, xi = [], x
        for r, ab in enumerate(arities):
            ev = take(2 << ab)
            xi >>= ab
            sib = [take(4) for _ in range(max(0, log_m - sum(arities[:r + 1]) - fp.cap_height))]
            assert g2.verify_merkle_proof_to_cap(ev, xi, caps[r], sib)
            steps.append([g2.Ext(ev[2 * k], ev[2 * k + 1]) for k in range(1 << ab)])
        fb = []
        for (pt, ranges), vals in zip(inst.batches, opened):
            at_x = [rows[o][c] for o, b, e in ranges for c in range(b, e)]          # salt words never enter (unsalted_eval)
            fb.append((g2.Ext(*pt), at_x, vals))
        assert g2.fri_verify_query(x, log_n, fp.rate_bits, arities, alpha, fb, rows, steps, betas, final_poly) is None
    assert pos[0] == len(pf)


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_case_is_proved_and_accepted_by_every_reading(case):
    inst = fc.build(case)
    och = fc.challenger(case)
    pf = _oracle.fri_prove_openings(inst.oracles, inst.batches, inst.log_n, inst.fp, och)
    assert _oracle.fri_verify_openings(pf, *inst.verifier_args(), fc.challenger(case)) == 0
    stage, ch_after = _verify.lib_fri_verify(pf, *inst.verifier_args(), fc.challenger(case))
    assert stage == 0
    assert ch_after == bytes(och)                   # the library's verifier leaves the transcript where the prover left it
    if inst.log_n <= 11:
        python_reading_accepts(inst, pf)
    # what the ids promise
    n = 1 << inst.log_n
    if case.id.startswith("zero_point"):
        # the opened values at zero are the constant terms
        k0 = sum(e - b for _, b, e in inst.batches[0][1])
        consts = np.concatenate([inst.oracles[o].coeffs[b:e, 0] for o, b, e in inst.batches[0][1]])
        assert (pf[8:8 + 2 * k0:2] == consts).all() and not pf[9:9 + 2 * k0:2].any()
    if case.id == "structured-all_zero":
        w, k = inst.witness_index(), sum(e - b for _, ranges in inst.batches for _, b, e in ranges)
        assert not pf[8:8 + 2 * k].any() and not pf[w - 2 * int(pf[2]):w].any()         # opened values and final polynomial: zero
    if case.id == "points-minus_one_nth":
        assert pow(case.point[0], n, fc.P) == fc.P - 1


def test_table_covers_what_it_names():
    ids = [c.id for c in fc.CASES]
    assert len(set(ids)) == len(ids)
    stress = [fc.stress_config(s)[0] for s in fc.STRESS_SEEDS]
    assert len(stress) == 8
    assert any(c["mixed"] for c in stress) and any(c["cap_height"] == 0 for c in stress)
    assert any(w <= 4 and s for c in stress for w, s in zip(c["widths"], c["salted"]))
    by = fc.BY_ID
    assert by["no_rounds"].fri["arities"] == [] and fc.fri_params(by["no_rounds"]).n_rounds == 0
    for cid, log_n in (("cap8_last_layer-10", 10), ("cap8_last_layer-11", 11)):
        c = by[cid]
        assert log_n + c.rate_bits - sum(c.fri["arities"]) == c.cap_height == 8       # the last layer has exactly 2^cap_height leaves
    for cid in ("pending_challenger-in", "pending_challenger-out"):
        ch = fc.challenger(by[cid])
        assert (ch.n_in, ch.n_out > 0) == ((1, False) if cid.endswith("in") else (0, True)), (cid, ch.n_in, ch.n_out)


def test_pow_scan_finds_every_launch_class():
    """the prefix seeds that tests/test_gpu_fri_edges.py grinds past the first launch: witnesses as measured when the table was written"""
    want = {0: {1: (1, 6097), 2: (0, 8995)}, 1: {1: (11, 5599), 2: (0, 11041)}}
    for rule in (0, 1):
        found = fc.pow_scan(rule)
        assert sorted(found) == [0, 1, 2], (rule, found)
        for cls in (1, 2):
            assert found[cls] == want[rule][cls], (rule, cls, found)
        assert found[0][1] >> fc.POW_LAUNCH_BITS == 0
