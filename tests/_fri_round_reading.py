"""A Python reading of the data a circuit that checks whole FRI query rounds is fed: the checker of sipp_amd/fri_verifier.py's inputs.  It
shares nothing with that module.  round_data(inst, proof) walks a flat opening proof (sipp_fri_prove_openings / oracle/fri.c) the way
tests/_fri_fold_reading.fold_data does and keeps what that function drops: the caps, every opened row, every sibling list, every
round's evaluations and coset siblings.  Every Merkle path is checked in Python integers with the oracle's host Poseidon
(oracle/py/plonky2_generic.py), every query by fri_verify_query."""
from oracle.py import plonky2_generic as g2

P = 0xFFFFFFFF00000001


def round_data(inst, proof):
    """-> (args, shape, data) of a flat opening proof of the tests/_fri_cases instance.
    data: the proof as a caller has it -- caps, points, opened, alpha, round_caps, betas, final_poly, queries = [(x_index, the opened
    row of every oracle, every oracle's siblings, per round the ext evaluations, per round the coset leaf's siblings)].
    args: (alpha, points, opened, caps, round_caps, betas, final_poly, x_indices, [(rows, siblings, evals, coset_siblings)]).
    shape: (log_m, cap_height, oracle widths, batches as column lists, arity_bits, n_rounds, final_len, n_queries)."""
    case, fp, log_n = inst.case, inst.fp, inst.log_n
    pf = [int(x) for x in proof]
    arities = [fp.arity_bits[i] for i in range(fp.n_rounds)]
    assert len(set(arities)) == 1 and not any(inst.n_salt)
    log_m, ch_ = log_n + fp.rate_bits, fp.cap_height
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
    round_caps, betas = [], []
    for _ in arities:
        round_caps.append([take(4) for _ in range(1 << ch_)])
        ch.observe_cap(round_caps[-1])
        betas.append(ch.get_ext())
    final_poly = [g2.Ext(*take(2)) for _ in range((1 << log_n) >> sum(arities))]
    for c in final_poly:
        ch.observe_ext(c)
    take(1)                                                          # the proof-of-work witness: not this circuit's
    g2.pow_response(ch, fp.pow_rule, pf[pos[0] - 1])
    caps = [[[int(v) for v in d] for d in o.cap] for o in inst.oracles]
    first = [sum(o.ncols for o in inst.oracles[:k]) for k in range(len(inst.oracles))]
    batches = [[first[o] + c for o, b, e in ranges for c in range(b, e)] for _, ranges in inst.batches]
    queries = []
    for _ in range(fp.num_queries):
        x = ch.get() % (1 << log_m)
        rows, sibs = [], []
        for o, cap in zip(inst.oracles, caps):
            row, sib = take(o.ncols), [take(4) for _ in range(log_m - ch_)]
            assert g2.verify_merkle_proof_to_cap(row, x, cap, sib)
            rows.append(row); sibs.append(sib)
        steps, evals, csibs, xi = [], [], [], x
        for r, ab in enumerate(arities):
            ev = take(2 << ab)
            xi >>= ab
            sib = [take(4) for _ in range(log_m - sum(arities[:r + 1]) - ch_)]
            assert g2.verify_merkle_proof_to_cap(ev, xi, round_caps[r], sib)
            steps.append([g2.Ext(ev[2 * k], ev[2 * k + 1]) for k in range(1 << ab)])
            evals.append([(ev[2 * k], ev[2 * k + 1]) for k in range(1 << ab)])
            csibs.append(sib)
        fb = []
        for (pt, ranges), vals in zip(inst.batches, opened):
            fb.append((g2.Ext(*pt), [rows[o][c] for o, b, e in ranges for c in range(b, e)], vals))
        assert g2.fri_verify_query(x, log_n, fp.rate_bits, arities, alpha, fb, rows, steps, betas, final_poly) is None
        queries.append((x, rows, sibs, evals, csibs))
    assert pos[0] == len(pf)
    pair = lambda v: (int(v[0]), int(v[1]))
    data = {"caps": caps, "points": [pair(g2.Ext(*pt)) for pt, _ in inst.batches], "opened": [[pair(v) for v in vals] for vals in opened],
            "alpha": pair(alpha), "round_caps": round_caps, "betas": [pair(b) for b in betas], "final_poly": [pair(c) for c in final_poly],
            "queries": queries}
    args = (data["alpha"], data["points"], data["opened"], caps, round_caps, data["betas"], data["final_poly"], [q[0] for q in queries],
            [q[1:] for q in queries])
    shape = (log_m, ch_, [o.ncols for o in inst.oracles], batches, arities[0], len(arities), len(final_poly), fp.num_queries)
    return args, shape, data
