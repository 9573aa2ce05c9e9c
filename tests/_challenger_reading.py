"""A Python reading of what a circuit that draws FRI's challenges itself must hold: the checker of sipp_amd/fri_proof.py.  It shares
nothing with that module.

  base_sum_row      SIPP_GEN_BASE_SUM (kind 15, include/sipp_hip.h) in exact integers: w[0] = sum_l w[1 + l] 2^(bits l) mod p, the limbs
                    taken as field values.  Importing this module registers it in tests._witness_reading.READINGS.
  arriving          the transcript a tests/_fri_cases case hands over, as (12 state words, pending inputs)
  drawn             alpha, every beta_r, the proof-of-work response, every x_index, the cap indices and the within indices of a flat
                    opening proof behind an arriving transcript, with the oracle's Challenger (oracle/py/plonky2_generic.py)
  invalid_witness   the value nearest to a proof's witness that is NOT a valid proof-of-work witness"""
from oracle.py import plonky2_generic as g2
from tests import _witness_reading as rd

P = 0xFFFFFFFF00000001
GEN_BASE_SUM = 15


def base_sum_row(w, n_limbs, bits):
    """one row's wires as a list of ints, in place"""
    w[0] = sum((w[1 + l] % P) << (bits * l) for l in range(n_limbs)) % P


rd.READINGS[GEN_BASE_SUM] = rd._row_by_row(lambda w, p, c: base_sum_row(w, p[0], p[1]))


def arriving(case):
    """-> ((the 12 state words, the pending inputs), the pending outputs) of the challenger the case's transcript leaves"""
    ch = g2.Challenger()
    ch.observe_many(list(case.prefix))
    for _ in range(case.gets):
        ch.get()
    return (list(ch.state), list(ch.input)), list(ch.output)


def _challenger(transcript):
    ch = g2.Challenger()
    ch.state, ch.input = [int(v) for v in transcript[0]], [int(v) for v in transcript[1]]
    return ch


def _to_the_witness(proof, transcript, n_opened, n_rounds, cap_height, final_len):
    """the challenger in front of the proof of work -> (it, alpha, betas, the witness's position)"""
    pf, at = [int(v) for v in proof], 8
    ch = _challenger(transcript)
    ch.observe_many(pf[at:at + 2 * n_opened])
    at += 2 * n_opened
    alpha = tuple(ch.get_n(2))
    betas = []
    for _ in range(n_rounds):
        ch.observe_many(pf[at:at + (4 << cap_height)])
        at += 4 << cap_height
        betas.append(tuple(ch.get_n(2)))
    ch.observe_many(pf[at:at + 2 * final_len])
    return ch, alpha, betas, at + 2 * final_len


def drawn(proof, transcript, log_m, cap_height, n_opened, arity_bits, n_rounds, final_len, n_queries, pow_rule):
    """-> {alpha, betas, witness, response, challenges (the full words the indices are cut from), x_index, cap_index, within}"""
    ch, alpha, betas, at = _to_the_witness(proof, transcript, n_opened, n_rounds, cap_height, final_len)
    witness = int(proof[at])
    response = g2.pow_response(ch, pow_rule, witness)
    challenges = ch.get_n(n_queries)
    x = [c % (1 << log_m) for c in challenges]
    return {"alpha": alpha, "betas": betas, "witness": witness, "response": response, "challenges": challenges, "x_index": x,
            "cap_index": [v >> (log_m - cap_height) for v in x],
            "within": [[(v >> (arity_bits * r)) & ((1 << arity_bits) - 1) for r in range(n_rounds)] for v in x]}


def invalid_witness(proof, transcript, cap_height, n_opened, n_rounds, final_len, pow_rule, pow_bits):
    """the value nearest to the proof's witness (above first) whose response has fewer than pow_bits leading zeros"""
    ch, _, _, at = _to_the_witness(proof, transcript, n_opened, n_rounds, cap_height, final_len)
    witness = int(proof[at])
    assert pow_bits > 0 and g2.pow_ok(g2.pow_response(ch.copy(), pow_rule, witness), pow_bits)
    for d in range(1, 1 << 16):
        for w in ((witness + d) % P, (witness - d) % P):
            if not g2.pow_ok(g2.pow_response(ch.copy(), pow_rule, w), pow_bits):
                return w
    raise AssertionError("no invalid witness nearby")
