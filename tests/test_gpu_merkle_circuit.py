"""Merkle openings in the outer circuit on the device: the swap Poseidon generator (SIPP_GEN_POSEIDON_SWAP) on all three launch paths
against the Python reading (tests/_witness_reading.py) cell for cell; a commitment made by the library opened through MerkleOpeningProver
(sipp_amd/merkle.py), proved word for word as the oracle proves the read witness, accepted by both verifiers, refused for every tampering."""
import ctypes as C

import numpy as np
import pytest

from sipp_amd import merkle as mk
from tests import _merkle_reading as mr
from tests import _oracle
from tests import _witness_reading as rd
from tests._device import NO_GRAPH, dev, first_mismatch, host, levels, run_levels
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

pytestmark = pytest.mark.gpu

P = _oracle.P
LAY = mk.SWAP_LAYOUT
SHIFTED = {"in_": 40, "out": 5, "swap": 17, "delta": 0, "sbox": 60}
DIGEST = (61, 62, 63, 64)
LEAF_LEN, LOG_N_TREE, CAP_H, N_PATHS = 16, 12, 4, 28
HEIGHT = LOG_N_TREE + 1 - CAP_H
ROUTES = (NO_GRAPH, 0, 0)                     # launch by launch, then the captured graph and its replay


def swap_gen(lay, sel=0, row=5):
    return (mk.GEN_POSEIDON_SWAP, sel, row, lay["in_"], lay["out"], lay["sbox"], lay["swap"], lay["delta"])


def table(rng, num_wires, n, lay, swap_rows):
    w = _oracle.rand_field(rng, (num_wires, n))
    w[lay["swap"], swap_rows] = rng.integers(0, 2, size=len(swap_rows), dtype=np.uint64)
    return w


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=3 << 30)
    yield c
    c.close()


@pytest.mark.parametrize("lay,num_wires", [(LAY, 135), (SHIFTED, 170)], ids=["upstream", "shifted"])
def test_row_local_swap_generator_matches_the_reading(ctx, lay, num_wires):
    """sipp_plonk_generate_witness, one lane per row, 2^12 rows: swap rows (swap 0 and 1) get the reading's deltas, S-box inputs and
    outputs; rows of another selector value stay as they were"""
    log_n, n = 12, 1 << 12
    rng = np.random.default_rng(11)
    sel = np.where(np.arange(n) % 3 == 1, 7, 5).astype(np.uint64).reshape(1, n)
    w = table(rng, num_wires, n, lay, np.flatnonzero(sel[0] == 5))
    gens = [swap_gen(lay)]
    want = rd.row_local(w, sel, gens, None)
    assert (want[:, sel[0] == 7] == w[:, sel[0] == 7]).all()
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, dev(sel), log_n, gens)
    assert first_mismatch(host(d_w), want) is None


def test_wide_level_of_swap_rows_matches_the_reading(ctx):
    """one level of 16384 swap rows (the one-lane level kernel), rows of another selector in between"""
    log_n, n = 15, 1 << 15
    rng = np.random.default_rng(12)
    sel = np.where(np.arange(n) % 2 == 0, 5, 7).astype(np.uint64).reshape(1, n)
    rows = np.flatnonzero(sel[0] == 5)
    assert len(rows) >= 16384
    w = table(rng, 135, n, LAY, rows)
    run_levels(ctx, w, sel, log_n, [swap_gen(LAY)], levels([rows]), ROUTES)


def test_chain_of_thin_swap_levels_matches_the_reading(ctx):
    """256 chains of 16 links (thin levels: sixteen lanes per row): link j's outputs 0 .. 3 become link j + 1's inputs 0 .. 3 or 4 .. 7"""
    log_n, n, chains, links = 12, 1 << 12, 256, 16
    rng = np.random.default_rng(13)
    sel = np.full((1, n), 5, dtype=np.uint64)
    row = rng.permutation(n)[:chains * links].reshape(links, chains)
    w = table(rng, 135, n, LAY, np.arange(n))
    side = rng.integers(0, 2, size=(links, chains))
    copies = []
    for j in range(links):
        cj = []
        if j + 1 < links:
            for c in range(chains):
                for t in range(4):
                    cj.append(((LAY["out"] + t) * n + int(row[j, c]), (LAY["in_"] + 4 * int(side[j + 1, c]) + t) * n + int(row[j + 1, c])))
        copies.append(cj)
    want = run_levels(ctx, w, sel, log_n, [swap_gen(LAY)], levels(list(row), copies), ROUTES)
    k = int(row[links - 1, 0])                                           # the last link read what the chain fed it
    assert (want[LAY["in_"] + 4 * int(side[-1, 0]):LAY["in_"] + 4 * int(side[-1, 0]) + 4, k] == want[LAY["out"]:LAY["out"] + 4, int(row[-2, 0])]).all()


@pytest.mark.parametrize("count", [1024, 16384], ids=["thin", "wide"])
def test_level_mixing_plain_and_swap_poseidon_rows_matches_the_reading(ctx, count):
    """kind 8 (its own layout, selector value 4) and kind 9 (upstream's, value 5) rows interleaved in one level: every row runs its own
    generator on either kernel, as the one-lane reading does"""
    log_n = 15
    n = 1 << log_n
    rng = np.random.default_rng(14)
    sel = np.full((1, n), 7, dtype=np.uint64)
    rows = np.sort(rng.permutation(n)[:count])
    sel[0, rows] = np.where(rng.integers(0, 2, size=count) == 1, 5, 4).astype(np.uint64)
    w = table(rng, 136, n, LAY, rows)
    gens = [(8, 0, 4, 100, 0, 30, 0, 0), swap_gen(LAY)]
    want = run_levels(ctx, w, sel, log_n, gens, levels([rows]), ROUTES)
    assert (want[:, sel[0] == 7] == w[:, sel[0] == 7]).all()


def test_bad_swap_layouts_are_refused_and_the_ctx_still_generates(ctx):
    import sipp_amd
    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(15)
    sel = np.full((1, n), 5, dtype=np.uint64)
    w = table(rng, 135, n, LAY, np.arange(n))
    d_w, d_c = dev(w), dev(sel)
    for bad in (dict(LAY, out=6), dict(LAY, delta=10), dict(LAY, sbox=20), dict(LAY, swap=40), dict(LAY, sbox=30), dict(LAY, swap=135),
                dict(LAY, delta=132)):
        with pytest.raises(sipp_amd.SippError) as e:
            ctx.plonk_generate_witness(d_w, d_c, log_n, [swap_gen(bad)])
        assert e.value.code == -1, bad
        assert (host(d_w) == w).all()
    ctx.plonk_generate_witness(d_w, d_c, log_n, [swap_gen(LAY)])
    assert first_mismatch(host(d_w), rd.row_local(w, sel, [swap_gen(LAY)], None)) is None


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def commitment(ctx):
    """random columns committed on the device (sipp_commit_batch_ex) and by the oracle: the same cap; openings from the oracle's tree"""
    rng = np.random.default_rng(16)
    cols = _oracle.rand_field(rng, (LEAF_LEN, 1 << LOG_N_TREE))
    _or, cap, _keep = ctx.commit_ex(dev(cols), LOG_N_TREE, 1, CAP_H)
    b = _oracle.Batch(cols, LOG_N_TREE, rate_bits=1, cap_height=CAP_H)
    assert (cap == b.cap).all()
    return cap, b, rng


@pytest.fixture(scope="module")
def prover(commitment):
    import sipp_amd
    mc = mk.MerkleOpeningCircuit(LEAF_LEN, HEIGHT, CAP_H, N_PATHS)
    ofp = fri(mc.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp = to_params(ofp)
    gp = sipp_amd.PlonkParams(80, 8, 2)
    gc = sipp_amd.PlonkCircuit.from_dict(mc.circuit())
    ws = sipp_amd.lib().sipp_circuit_workspace_bytes(mc.log_n, C.byref(gp), C.byref(gfp), C.byref(gc))
    c = sipp_amd.Ctx(workspace_bytes=ws)
    pr = mk.MerkleOpeningProver(c, LEAF_LEN, HEIGHT, CAP_H, N_PATHS, fri=gfp, digest=DIGEST)
    yield pr, c, ofp
    pr.close()
    c.close()


def _verdicts(pr, ofp, pf):
    cs_cap = pr.cap
    return pr.verify(pf), _oracle.plonk_verify_gates(pf, cs_cap, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST)


def test_openings_of_a_device_commitment_prove_and_verify(ctx, commitment, prover):
    import sipp_amd
    cap, b, rng = commitment
    pr, c, ofp = prover
    mc = pr.circ
    cs = mc.constants_sigmas()
    assert (pr.cap == _oracle.Batch(cs, mc.log_n, rate_bits=3, cap_height=4).cap).all()
    for round_ in range(2):                                        # a second opening set through the same circuit data
        idx = [int(x) for x in rng.integers(0, 1 << (LOG_N_TREE + 1), size=N_PATHS)]
        leaves, sib = mr.opening(b, idx, HEIGHT)
        pis = mc.public_inputs(cap, idx, leaves)
        pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
        pw = mc.partial_witness(cap, idx, leaves, sib)
        want = rd.replay(pw, cs[:4], mc.generators(), pih, mc.schedule())
        if round_ == 0:                                            # the device witness (the generation CircuitData.prove runs) = the reading
            d_w = dev(pw)
            ctx.plonk_generate_witness_levels(d_w, dev(cs[:4]), mc.log_n, mc.generators(), pih, sipp_amd.PlonkSchedule.from_dict(mc.schedule()))
            assert first_mismatch(host(d_w), want) is None
        pf = pr.prove(cap, idx, leaves, sib)
        ref = _oracle.plonk_prove_gates(want, cs, mc.log_n, _oracle.plonk_params(80, 8, 2), ofp, pr.circuit, DIGEST, pis)
        assert len(pf) == len(ref) and (pf == ref).all(), round_
        assert _verdicts(pr, ofp, pf) == ((0, 0), 0)


@pytest.mark.parametrize("tamper", ["sibling", "leaf", "index_bit", "cap_word"])
def test_tampered_openings_are_refused_and_the_prover_goes_on(commitment, prover, tamper):
    cap, b, _ = commitment
    pr, c, ofp = prover
    rng = np.random.default_rng(17)
    idx = [int(x) for x in rng.integers(0, 1 << (LOG_N_TREE + 1), size=N_PATHS)]
    leaves, sib = mr.opening(b, idx, HEIGHT)
    cap2 = cap.copy()
    if tamper == "sibling":
        sib[2, 5, 0] ^= np.uint64(1)
    elif tamper == "leaf":
        leaves[4, 13] ^= np.uint64(1)
    elif tamper == "index_bit":
        idx[6] ^= 1 << 2
    else:
        cap2[idx[8] >> HEIGHT, 1] ^= np.uint64(1)                    # a word path 8 selects
    pf = pr.prove(cap2, idx, leaves, sib)
    (st, stage), orc = _verdicts(pr, ofp, pf)
    assert st != 0 and orc != 0, (st, stage, orc)
    good = pr.prove(cap, idx, *mr.opening(b, idx, HEIGHT))
    assert _verdicts(pr, ofp, good) == ((0, 0), 0)
