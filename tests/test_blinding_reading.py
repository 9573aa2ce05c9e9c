"""Zero-knowledge blinding without a GPU: the random function of tests/_blinding_cases.py against two other readings, plonky2's counting
rule at hand-computed shapes, the builder's blinding rows, and one "SIPPPLK5" proof (tests/golden/blinding_proof_small.npz, written on a
GPU by tools/capture_blinding_fixture.py) through the library's host verifier and the composed reading: accepted as it is, refused at
the stage each kind of damage belongs to."""
import hashlib
import os
import sys

import numpy as np
import pytest

from tests import _blinding_cases as bc
from tests import _oracle as orc

P = bc.P
D, NC = 8, 2


# ---- the random function -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, (1 << 33) - 1])
@pytest.mark.parametrize("counter", [0, (1 << 32) + 1])
@pytest.mark.parametrize("seed", [(0, 0, 0, 0), (P - 1, P - 1, P - 1, P - 1)], ids=["zero_seed", "seed_words_p_minus_1"])
def test_block_is_hash_n_to_m_no_pad_and_the_oracles_permutation(seed, counter, index):
    sys.path.insert(0, os.path.join(bc.ROOT, "oracle", "py"))
    import plonky2_generic as pg
    for stream in range(4):
        got = bc.block(seed, counter, stream, index)
        assert len(got) == 8 and all(0 <= x < P for x in got)
        assert got == pg.hash_n_to_m_no_pad(list(seed) + [counter, stream, index], 8)
        assert got == [int(x) for x in orc.permute(list(seed) + [counter, stream, index, 0, 0, 0, 0, 0])[:8]]


def test_the_bulk_reading_is_block_and_the_columns_follow_the_rule():
    cols = bc.salt_columns(bc.SEED, 7, bc.STREAM_ZS, 16)
    for j in (0, 1, 6, 15):
        assert [int(cols[k][j]) for k in range(4)] == bc.block(bc.SEED, 7, bc.STREAM_ZS, j >> 1)[4 * (j & 1): 4 * (j & 1) + 4]
    nat = bc.salt_natural(bc.SEED, 7, bc.STREAM_ZS, 4)
    assert (nat[:, 1] == cols[:, 8]).all() and (nat[:, 3] == cols[:, 12]).all() and (nat[:, 15] == cols[:, 15]).all()
    assert not (bc.salt_columns(bc.SEED, 8, bc.STREAM_ZS, 16) == cols).any()
    assert not (bc.salt_columns(bc.SEED, 7, bc.STREAM_WIRES, 16) == cols).any()


def test_blind_fill_follows_the_rule():
    w = np.full((12, 8), 5, dtype=np.uint64)
    consts = np.array([[9, 3, 9, 9, 9, 9, 9, 3]], dtype=np.uint64)
    out, mask = bc.blind_fill(w, consts, [(bc.GEN_RANDOM, 0, 3, 7, 3, 0, 0, 0)], bc.SEED, 2)
    assert mask.sum() == 6 and (out[~mask] == 5).all()
    assert int(out[7][7]) == bc.block(bc.SEED, 2, 0, (7 << 9) + 0)[7]
    assert int(out[8][7]) == bc.block(bc.SEED, 2, 0, (7 << 9) + 1)[0] and int(out[9][1]) == bc.block(bc.SEED, 2, 0, (1 << 9) + 1)[1]


# ---- the counting rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, want", [
    ((2, [2, 2, 2], 10), (70, 72, 74)),        # queries 2, three rounds of arity 4, final length 16: 2 (1 + 2 * 9 + 16)
    ((28, [4, 4, 4], 18), (4340, 4342, 4344)),  # 28 queries, three rounds of arity 16, final length 64: 28 (1 + 2 * 45 + 64)
    ((1, [], 3), (9, 11, 13)),                 # no round: the whole polynomial is the final one: 1 + 0 + 8
], ids=["q2_arity4x3_final16", "q28_arity16x3_final64", "no_rounds"])
def test_blinding_counts_at_hand_computed_shapes(shape, want):
    from sipp_amd import circuit
    q, arity, log_n = shape
    fri = {"num_queries": q, "n_rounds": len(arity), "arity_bits": arity}
    assert circuit.blinding_counts(fri, log_n) == want[1:]
    assert bc.blinding_counts(q, arity, log_n) == want[1:]
    assert want[1] == 2 + want[0] and want[2] == 4 + want[0]
    assert circuit.blinding_counts(fri, log_n, regular=5) == (5, want[2]) and circuit.blinding_counts(fri, log_n, z=0) == (want[1], 0)
    fp = bc.proof_fri(10)
    if shape[2] == 10:
        assert circuit.blinding_counts(fp, 10) == want[1:]          # the struct the prover takes, as well as a dict


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
def outputs_digest(c):
    h = hashlib.sha256()
    circ = c.circuit()
    for k in sorted(circ):
        v = circ[k]
        h.update(k.encode())
        h.update(np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    h.update(repr(c.generators()).encode())
    s = c.schedule()
    for k in sorted(s):
        h.update(k.encode())
        h.update(np.asarray(s[k]).tobytes())
    h.update(np.ascontiguousarray(c.constants_sigmas()).tobytes())
    h.update(repr((c.log_n, c.rows_used, c.n_levels)).encode())
    return h.hexdigest()


def test_with_blinding_off_the_builder_is_bit_identical():
    """the digest of every output of tests/_lookup_tables_circuit.py's circuit, recorded with the builder as it was before it had
    blinding; and a circuit that declares the Blind gate but no blinding carries no row and no generator of it"""
    from tests._lookup_tables_circuit import XorLookupCircuit
    assert outputs_digest(XorLookupCircuit()) == "0e2350aee33615f29852049b2e069a11499a778fcef847679ba00fb4e3457d09"
    off = bc.circuit(True, blind=False)
    assert off.blinding == (0, 0) and not (off.gate == off.BLIND).any()
    assert all(g[0] != bc.GEN_RANDOM for g in off.generators())


@pytest.mark.parametrize("lookups", [False, True], ids=["no_lookups", "lookups"])
def test_with_blinding_on_the_rows_are_there(lookups):
    off, on = bc.circuit(lookups, blind=False), bc.circuit(lookups)
    regular, z = bc.blinding_counts(2, [2, 2, 2], 10)
    assert on.log_n == 10 and on.blinding == (regular, z) == (72, 74)
    assert on.rows_used == off.rows_used + regular + 2 * z
    assert len(on.blind_rows["regular"]) == regular and len(on.blind_rows["pairs"]) == z
    blind_rows = sorted(on.blind_rows["regular"] + [r for pair in on.blind_rows["pairs"] for r in pair])
    assert blind_rows == list(range(off.rows_used, on.rows_used))                      # behind the circuit's rows
    assert (on.gate[blind_rows] == on.BLIND).all() and on.BLIND != 0
    assert (on.gate[on.rows_used:] == 0).all() and (on.c0[on.rows_used:] == 0).all()  # padding: Noop rows of zeros
    # the gate: a selector value of its own, no constraints, SIPP_GEN_RANDOM over every wire
    g = on.circuit()["gates"][on.BLIND]
    assert g[1] == on.BLIND and g[5] == 0
    assert [x for x in on.generators() if x[0] == bc.GEN_RANDOM] == [(bc.GEN_RANDOM, g[0], on.BLIND, 0, on.num_wires, 0, 0, 0)]
    assert len(on.generators()) == len(off.generators()) + 1 <= 32
    cs = on.constants_sigmas()
    assert (cs[g[0]][blind_rows] == on.BLIND).all() and int((cs[g[0]] == on.BLIND).sum()) == len(blind_rows)
    # what the circuit had before is where it was
    assert (on.gate[:off.rows_used] == off.gate[:off.rows_used]).all()
    # every pair: routed wire w of the two rows is ONE copy class of exactly those two cells, copied at level 0 into a level-1 row
    n, R = on.n, on.num_routed
    cycles = {tuple(c) for c in on.cycles}
    sched = on.schedule()
    copies = set(zip(sched["copy_src"].tolist(), sched["copy_dst"].tolist()))
    for a, b in on.blind_rows["pairs"]:
        assert sched["row_level"][a] == 0 and sched["row_level"][b] == 1
        for w in (0, 1, R - 1):
            assert (w * n + a, w * n + b) in cycles and (w * n + a, w * n + b) in copies
    for r in on.blind_rows["regular"]:
        assert sched["row_level"][r] == 0
    pair_cells = {w * n + r for pair in on.blind_rows["pairs"] for r in pair for w in range(R)}
    assert sum(len(c) for c in on.cycles if c[0] in pair_cells) == len(pair_cells) == 2 * R * z
    # the sigmas swap the two cells
    a, b = on.blind_rows["pairs"][0]
    sig = cs[on.num_constants:]
    ident = lambda w, r: pow(7, w, P) * pow(pow(bc.lc.ROOT32, 1 << (32 - on.log_n), P), r, P) % P
    assert int(sig[5][a]) == ident(5, b) and int(sig[5][b]) == ident(5, a)
    r = on.blind_rows["regular"][0]
    assert int(sig[5][r]) == ident(5, r)


def test_blinding_rows_that_cross_a_power_of_two_reach_a_stable_count():
    """arity 2 down to a final polynomial of 4, two queries: 24 + 2 * 26 rows at 2^5 do not fit 32 rows; at 2^7 the rule asks for
    32 + 2 * 34, which fit"""
    fri_of = lambda log_n: {"num_queries": 2, "n_rounds": log_n - 2, "arity_bits": [1] * (log_n - 2)}
    off = bc.BlindCircuit(lookups=False, blind=False, min_log_n=5)
    on = bc.BlindCircuit(lookups=False, min_log_n=5, fri_of=fri_of)
    assert off.log_n == 5 and bc.blinding_counts(2, [1] * 3, 5) == (24, 26) and off.rows_used + 24 + 52 > 64
    assert on.log_n == 7 and on.blinding == bc.blinding_counts(2, [1] * 5, 7) == (32, 34)
    assert on.rows_used == off.rows_used + 32 + 68 <= 128
    # the counts by keyword: no loop needed
    fixed = bc.BlindCircuit(lookups=False, min_log_n=5, fri_of=fri_of, regular=3, z=2)
    assert fixed.log_n == 5 and fixed.blinding == (3, 2) and fixed.rows_used == off.rows_used + 7


def test_the_prover_wrapper_refuses_parameters_that_need_more_rows():
    from sipp_amd.circuit import CircuitProver, fri_params
    short = bc.BlindCircuit(lookups=False, regular=3, z=2)
    with pytest.raises(ValueError):
        CircuitProver(None, short, fri=bc.proof_fri(short.log_n, 0), zero_knowledge=True, seed=bc.SEED)
    with pytest.raises(ValueError):                                  # 28 queries need more rows than 72 + 2 * 74
        CircuitProver(None, bc.circuit(False), fri=fri_params(10, num_queries=28), zero_knowledge=True, seed=bc.SEED)
    with pytest.raises(ValueError):                                  # no blinding rows at all
        CircuitProver(None, bc.circuit(False, blind=False), fri=bc.proof_fri(10, 0), zero_knowledge=True, seed=bc.SEED)


# ---- the committed proof ---------------------------------------------------------------------------------------------------------------------
class Fixture:
    def __init__(self):
        import sipp_amd
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blinding_proof_small.npz"))
        self.proof, self.cap = z["proof"], z["cap"]
        assert tuple(int(x) for x in z["seed"]) == bc.SEED
        self.c = bc.circuit(True)
        self.a, self.b = (int(x) for x in z["inputs"])
        self.circ = self.c.circuit()
        self.desc = tuple(self.circ["lookup"])
        self.pc = sipp_amd.PlonkCircuit.from_dict(self.circ)
        self.gp = sipp_amd.PlonkParams(self.c.num_routed, D, NC)
        self.fp, self.fp_plain = bc.proof_fri(10, 1), bc.proof_fri(10, 0)
        self.proof.setflags(write=False)

    def verdict(self, proof, fp=None):
        import sipp_amd
        return sipp_amd.plonk_verify_gates_lookup(proof, self.cap, self.gp, self.fp if fp is None else fp, self.pc, bc.PROOF_DIGEST, self.desc)

    def reading(self, proof, fp=None):
        return bc.read_proof5(proof, self.circ, self.cap, bc.PROOF_DIGEST, self.fp if fp is None else fp, D, NC, 1)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_the_fixture_is_accepted_by_the_verifier_and_by_the_reading(fx):
    p = fx.proof
    assert int(p[0]) == bc.MAGIC5 and int(p[1]) == 10 and int(p[12]) == 1 and [int(v) for v in p[16:24]] == list(fx.desc)
    assert len(p) * 8 < 64 << 10 and int(p[-1]) == fx.c.value(fx.a, fx.b)
    assert fx.verdict(p) == 0
    assert fx.reading(p) is None


def test_the_fixtures_query_leaves_carry_the_readings_salt(fx):
    rounds = bc.query_rounds(fx.proof, fx.circ, bc.PROOF_DIGEST, fx.fp, D, NC, 1)
    assert len(rounds) == 2
    for x, leaves, _ in rounds:
        for o, stream in ((1, bc.STREAM_WIRES), (2, bc.STREAM_ZS), (3, bc.STREAM_QUOTIENT)):
            assert leaves[o][-4:] == bc.block(bc.SEED, 0, stream, x >> 1)[4 * (x & 1): 4 * (x & 1) + 4], (x, o)


def test_a_changed_salt_word_of_a_query_leaf_is_refused(fx):
    """the Merkle path of that oracle's leaf no longer ends in its cap: stage 123 + oracle"""
    x, leaves, where = bc.query_rounds(fx.proof, fx.circ, bc.PROOF_DIGEST, fx.fp, D, NC, 1)[1]
    for o in (1, 2, 3):
        bad = fx.proof.copy()
        at = where[o] + len(leaves[o]) - 1                       # the last salt word
        assert int(bad[at]) == leaves[o][-1]
        bad[at] ^= np.uint64(1)
        assert fx.verdict(bad) == 123 + o
        got = fx.reading(bad)
        assert got is not None and got[0] == "fri"


def test_damage_to_the_header_is_refused_at_stage_201(fx):
    cleared = fx.proof.copy()
    cleared[12] = 0
    assert fx.verdict(cleared) == 201 and fx.reading(cleared) == "header"
    older = fx.proof.copy()
    older[0] = bc.MAGIC4
    assert fx.verdict(older) == 201 and fx.reading(older) == "header"
    assert fx.verdict(older, fx.fp_plain) == 201                  # nor is it a "SIPPPLK4" proof: header[12] is set
    older[12] = 0
    assert fx.verdict(older, fx.fp_plain) != 0                    # and with it cleared the leaves do not hash to the caps
    assert fx.verdict(fx.proof, fx.fp_plain) == 201 and fx.reading(fx.proof, fx.fp_plain) == "header"
    assert fx.verdict(fx.proof[:-1]) == 201 and fx.reading(fx.proof[:-1]) == "header"      # truncated by one word: header[5] is the length


def test_a_changed_public_input_is_refused(fx):
    """the public inputs are hashed into the transcript and into the PublicInput gate: the vanishing equation fails"""
    bad = fx.proof.copy()
    bad[-1] ^= np.uint64(1)
    assert fx.verdict(bad) == 210
    assert fx.reading(bad) == "vanishing"
