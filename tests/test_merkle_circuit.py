"""Merkle openings in the outer circuit on the CPU (sipp_amd/merkle.py): the swap Poseidon gate's program against the Python reading of its
row (tests/_merkle_reading.py) through oracle/plonk_gates.c; the opening circuit over a real commitment (_oracle.Batch) with the witness
replayed level by level, proved by the oracle and judged by both verifiers (the oracle's and the library's verify.cpp)."""
import numpy as np
import pytest

from sipp_amd import merkle as mk
from tests import _merkle_reading as mr
from tests import _witness_reading as rd
from tests import _oracle, _verify
from tests.test_oracle_plonk import fri

P = _oracle.P
LAY = mk.SWAP_LAYOUT
DIGEST = (51, 52, 53, 54)


def one_gate(prog, num_wires=135):
    return {"num_wires": num_wires, "num_routed": 80, "num_constants": 1, "num_selectors": 1, "gates": [(0, 0, 0, 1, 0, 123)],
            "programs": prog, "num_gate_constraints": 123}


def swap_rows(rng, n, swap_values, num_wires=135, lay=LAY):
    """n rows of random inputs, swap cell = swap_values (broadcast), the rest from the reading"""
    w = _oracle.rand_field(rng, (num_wires, n))
    w[lay["swap"]] = np.asarray(swap_values, dtype=np.uint64)
    mr.poseidon_rows(w, np.arange(n), lay["in_"], lay["out"], lay["sbox"], swap=lay["swap"], delta=lay["delta"])
    return w


def nonzero(circ, w, r):
    return set(np.flatnonzero(_oracle.plonk_gate_constraints_base(circ, w[:, r], np.zeros(1, dtype=np.uint64), [0, 0, 0, 0])).tolist())


def test_swap_gate_program_has_upstreams_123_constraints_in_order():
    """swap (swap - 1); swap (in[4+i] - in[i]) - delta_i; S-box inputs of rounds 1 .. 3, 4 .. 25, 26 .. 29; outputs -- each  form - wire"""
    prog = mk.poseidon_swap_gate()
    cons = mr.decode(prog, 0, 123)
    assert len(prog) == sum(1 + sum(2 + 2 * len(f) for _, f in c) for c in cons)
    sw, dl, sb, out = LAY["swap"], LAY["delta"], LAY["sbox"], LAY["out"]
    norm = lambda c: sorted((k, tuple(sorted(f))) for k, f in c)
    assert norm(cons[0]) == norm([(1, [(0, sw), (0, sw)]), (P - 1, [(0, sw)])])
    for i in range(4):
        assert norm(cons[1 + i]) == norm([(1, [(0, sw), (0, 4 + i)]), (P - 1, [(0, sw), (0, i)]), (P - 1, [(0, dl + i)])])
    targets = [sb + k for k in range(36)] + [sb + 36 + r for r in range(22)] + [sb + 58 + k for k in range(48)] + [out + i for i in range(12)]
    for j, t in enumerate(targets):
        c = cons[5 + j]
        assert (P - 1, [(0, t)]) in c, j                                     # state_form - wire
        assert max(len(f) for _, f in c) == 7
    # round 1 reads the swapped inputs: (in_i + delta_i + rc)^7 -- mixed monomials in two wires
    assert any(len(set(f)) == 2 for _, f in cons[5])
    assert all(len(set(f)) <= 1 for j in range(17, 123) for _, f in cons[j])


@pytest.mark.parametrize("lay", [LAY, {"in_": 40, "out": 5, "swap": 17, "delta": 0, "sbox": 60}], ids=["upstream", "shifted"])
def test_random_swap_rows_satisfy_every_constraint(lay):
    rng = np.random.default_rng(3)
    prog = mk.poseidon_swap_gate(**lay)
    circ = one_gate(prog, 170)
    for s in (0, 1):
        w = swap_rows(rng, 64, s, 170, lay)
        for r in range(64):
            assert not nonzero(circ, w, r), (s, r)


def test_tampered_swap_rows_fail_exactly_the_constraints_that_read_the_tampered_cell():
    rng = np.random.default_rng(4)
    circ = one_gate(mk.poseidon_swap_gate())
    w = swap_rows(rng, 8, 2)                                                 # swap = 2, deltas by the generator's formula
    for r in range(8):
        assert nonzero(circ, w, r) == {0}
    for i in range(4):
        w = swap_rows(rng, 4, [0, 1, 0, 1])
        w[LAY["delta"] + i] = (w[LAY["delta"] + i] + np.uint64(1)) % np.uint64(P)
        for r in range(4):
            bad = nonzero(circ, w, r)
            assert 1 + i in bad and not bad & ({0, 1, 2, 3, 4} - {1 + i})
    for i in range(12):
        w = swap_rows(rng, 2, [0, 1])
        w[LAY["out"] + i] ^= np.uint64(1 << 7)
        for r in range(2):
            assert nonzero(circ, w, r) == {111 + i}


# ---- the opening circuit -------------------------------------------------------------------------------------------------------------
LEAF_LEN, LOG_N_TREE, CAP_H, N_PATHS = 16, 12, 4, 28
HEIGHT = LOG_N_TREE + 1 - CAP_H                                              # 2^13 leaves (blowup 2), cap of 16


@pytest.fixture(scope="module")
def opening():
    rng = np.random.default_rng(5)
    cols = _oracle.rand_field(rng, (LEAF_LEN, 1 << LOG_N_TREE))
    b = _oracle.Batch(cols, LOG_N_TREE, rate_bits=1, cap_height=CAP_H)
    idx = [int(x) for x in rng.integers(0, 1 << (LOG_N_TREE + 1), size=N_PATHS)]
    leaves, sib = mr.opening(b, idx, HEIGHT)
    mc = mk.MerkleOpeningCircuit(LEAF_LEN, HEIGHT, CAP_H, N_PATHS)
    cs = mc.constants_sigmas()
    cs_cap = _oracle.Batch(cs, mc.log_n, rate_bits=3, cap_height=4).cap
    return {"cap": b.cap, "idx": idx, "leaves": leaves, "sib": sib, "mc": mc, "cs": cs, "cs_cap": cs_cap}


def witness(o, cap=None, idx=None, leaves=None, sib=None):
    mc = o["mc"]
    cap = o["cap"] if cap is None else cap
    idx = o["idx"] if idx is None else idx
    leaves = o["leaves"] if leaves is None else leaves
    sib = o["sib"] if sib is None else sib
    pis = mc.public_inputs(cap, idx, leaves)
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(mc.partial_witness(cap, idx, leaves, sib), o["cs"][:4], mc.generators(), pih, mc.schedule())
    return w, pis, pih


def prove_and_judge(o, w, pis):
    mc = o["mc"]
    op = _oracle.plonk_params(80, 8, 2)
    ofp = fri(mc.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    circ = mc.circuit()
    pf = _oracle.plonk_prove_gates(w, o["cs"], mc.log_n, op, ofp, circ, DIGEST, pis)
    return _oracle.plonk_verify_gates(pf, o["cs_cap"], op, ofp, circ, DIGEST), _verify.lib_plonk_verify(pf, o["cs_cap"], op, ofp, circ, DIGEST)


def test_opening_circuit_shape():
    mc = mk.MerkleOpeningCircuit(LEAF_LEN, HEIGHT, CAP_H, N_PATHS)
    circ = mc.circuit()
    assert [g[5] for g in circ["gates"]] == [0, 4, 1, 1 + HEIGHT, 2 * (CAP_H + 2), 123]
    # filter degree (group size - 1, + 1 for several selector columns) + gate degree <= max_degree = 8
    degrees = [0, 1, 1, 2, CAP_H + 1, 7]
    for (si, row, lo, hi, off, nc), d in zip(circ["gates"], degrees):
        cons = mr.decode(circ["programs"], off, nc)
        assert max([len(f) for c in cons for _, f in c] or [0]) == d
        assert (hi - lo - 1) + 1 + d <= 8
    assert mc.n_pi == 4 * 16 + N_PATHS * (2 + LEAF_LEN) and mc.n_levels == 1 + max(mc.n_pi_rows, 2 + HEIGHT)
    assert max(max(c) for c in mc.cycles) < 80 * mc.n
    cells = [x for c in mc.cycles for x in c]
    assert len(cells) == len(set(cells))                                     # every cell on one cycle at most


def test_opening_circuit_witness_satisfies_every_row_and_cycle_and_the_proof_verifies(opening):
    o, mc = opening, opening["mc"]
    w, pis, pih = witness(o)
    circ = mc.circuit()
    for r in range(mc.n):
        assert not _oracle.plonk_gate_constraints_base(circ, w[:, r], o["cs"][:4, r], pih).any(), (r, int(mc.gate[r]))
    flat = w.reshape(-1)
    for cyc in mc.cycles:
        assert len(set(flat[np.asarray(cyc, dtype=np.int64)].tolist())) == 1
    assert (w[12:16, mc.chain_row[-1]] == _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))).all()
    assert pis[:64] == [int(x) for x in o["cap"].reshape(-1)]
    assert prove_and_judge(o, w, pis) == (0, 0)


def _selected_cap_word(o):
    k = 3
    return (o["idx"][k] >> HEIGHT) * 4 + 2


@pytest.mark.parametrize("tamper", ["sibling", "leaf", "index_bit", "cap_word"])
def test_tampered_openings_give_proofs_both_verifiers_refuse(opening, tamper):
    o = opening
    kw = {}
    if tamper == "sibling":
        sib = o["sib"].copy()
        sib[5, 3, 1] ^= np.uint64(1)
        kw["sib"] = sib
    elif tamper == "leaf":
        leaves = o["leaves"].copy()
        leaves[7, 11] ^= np.uint64(1)
        kw["leaves"] = leaves
    elif tamper == "index_bit":
        idx = list(o["idx"])
        idx[9] ^= 1 << 4
        kw["idx"] = idx
    else:
        cap = o["cap"].copy().reshape(-1)
        cap[_selected_cap_word(o)] ^= np.uint64(1)
        kw["cap"] = cap.reshape(-1, 4)
    w, pis, _ = witness(o, **kw)
    orc, lib = prove_and_judge(o, w, pis)
    assert orc == -210 and lib == 210, (orc, lib)
