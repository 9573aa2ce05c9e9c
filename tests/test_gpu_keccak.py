"""Keccak-256 Merkle trees on the device (sipp_amd/csrc/keccak.hip) against the pure-Python reading of tests/_keccak_cases.py: leaves
over an LDE, FRI layer leaves and whole trees word for word; sipp_commit_batch_h against the generic reading's PolynomialBatch with its two
tree functions replaced; opening proofs of a few rows of tests/_fri_cases.py and whole outer proofs (plain, lookups, blinded, both) under
Keccak through the library's verifier and the reading's path checks; hasher 0 through every new entry equal to the entry it is a sibling
of; the refusals.  The shapes are the smallest at which these kernels can go wrong (the catalogue says why each is there)."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import _blinding_cases as bc
from tests import _fri_cases as fc
from tests import _keccak_cases as kc
from tests import _oracle
from tests._device import dev, host
from tests.test_gpu_fri_generic import to_params

pytestmark = pytest.mark.gpu
P = kc.P
D, NC = 8, 2
E_BADARG = -1


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=2 << 30)
    yield c
    c.close()


@pytest.fixture
def keccak_reading(monkeypatch):
    """oracle/py/plonky2_generic.py with hash_or_noop / two_to_one replaced by the Keccak ones; its Challenger stays Poseidon"""
    from oracle.py import plonky2_generic as g

    def draw():
        ch = g.Challenger()
        ch.observe_many([1, 2, 3, 4, 5])
        return ch.get_n(3)

    before = draw()
    monkeypatch.setattr(g, "hash_or_noop", kc.hash_or_noop)
    monkeypatch.setattr(g, "two_to_one", kc.two_to_one)
    assert draw() == before
    return g


def u64(t):
    return host(t)


def rand_cols(seed, ncols, n):
    return np.random.default_rng(seed).integers(0, P, size=(ncols, n), dtype=np.uint64)


# ---- leaves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_leaves, ncols", kc.LEAF_CASES, ids=["2^%d_x_%d" % c for c in kc.LEAF_CASES])
def test_leaves_word_for_word(ctx, log_leaves, ncols):
    lde = rand_cols(1000 * log_leaves + ncols, ncols, 1 << log_leaves)
    got = u64(ctx.merkle_leaves_h(dev(lde), log_leaves, "keccak"))
    assert got.shape == (1 << log_leaves, 4)
    for j in kc.checked_leaves(log_leaves):
        assert [int(v) for v in got[j]] == kc.hash_or_noop(int(v) for v in lde[:, j]), (j, ncols)


def test_leaves_of_non_canonical_words_hash_the_reduced_values(ctx):
    log_leaves, ncols = kc.NONCANONICAL_CASE
    lde = rand_cols(5, ncols, 1 << log_leaves)
    odd = [P, P + 1, (1 << 64) - 1, P + (1 << 32) - 2]
    for c in range(ncols):
        for j in range(c % 3, 1 << log_leaves, 3):
            lde[c, j] = odd[(c + j) % 4]
    lde3 = lde[:3].copy()
    for table in (lde, lde3):
        got = u64(ctx.merkle_leaves_h(dev(table), log_leaves, "keccak"))
        for j in range(1 << log_leaves):
            assert [int(v) for v in got[j]] == kc.hash_or_noop(int(v) % P for v in table[:, j]), j


def test_leaves_with_hasher_zero_are_the_poseidon_entry(ctx):
    for ncols in (3, 9):
        d = dev(rand_cols(9, ncols, 1 << 7))
        assert (host(ctx.merkle_leaves_h(d, 7, "poseidon")) == host(ctx.poseidon_leaves(d, 7))).all()


# ---- FRI layer leaves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_leaves, ab", kc.FRI_LEAF_CASES, ids=["2^%d_arity_bits_%d" % c for c in kc.FRI_LEAF_CASES])
def test_fri_layer_leaves_word_for_word(ctx, log_leaves, ab):
    n = 1 << (log_leaves + ab)
    vals = rand_cols(77 + ab, 2, n)
    vals[0, 1], vals[1, n - 1] = P + 3, (1 << 64) - 1                          # reduced before they are hashed, here too
    got = u64(ctx.fri_leaves_h(dev(vals), ab, "keccak"))
    assert got.shape == (1 << log_leaves, 4)
    for k in range(1 << log_leaves):
        leaf = [int(vals[i & 1, (k << ab) + (i >> 1)]) for i in range(2 << ab)]
        assert [int(v) for v in got[k]] == kc.hash_or_noop(leaf), k                 # arity 2: four words = 32 bytes, hashed


# ---- levels ---------------------------------------------------------------------------------------------------------------------------
def tree_of(ctx, digests, log_leaves, cap_height, hasher="keccak"):
    import torch
    n = 1 << log_leaves
    tree = torch.zeros((2 * n, 4), dtype=torch.int64, device="cuda")
    tree[:n] = dev(np.array(digests, dtype=np.uint64))
    cap = ctx.merkle_levels_h(tree, log_leaves, cap_height, hasher)
    return u64(tree), cap


def check_tree(ctx, digests, log_leaves, cap_height):
    tree, cap = tree_of(ctx, digests, log_leaves, cap_height)
    levels = kc.merkle_levels(digests, cap_height)
    at = 0
    for lvl in levels:
        assert [[int(v) for v in row] for row in tree[at:at + len(lvl)]] == lvl, "level of %d nodes" % len(lvl)
        at += len(lvl)
    assert [[int(v) for v in row] for row in cap] == levels[-1]


@pytest.mark.parametrize("log_leaves, cap_height", kc.LEVEL_CASES, ids=["2^%d_cap_%d" % c for c in kc.LEVEL_CASES])
def test_whole_trees_word_for_word(ctx, log_leaves, cap_height):
    rng = random.Random(31 * log_leaves + cap_height)
    check_tree(ctx, [kc.random_digest(rng) for _ in range(1 << log_leaves)], log_leaves, cap_height)


@pytest.mark.parametrize("log_leaves, cap_height", kc.SHORT_WIDE_LEVEL_CASES, ids=["2^%d_cap_%d" % c for c in kc.SHORT_WIDE_LEVEL_CASES])
def test_a_wide_launch_cut_short_by_the_cap(ctx, log_leaves, cap_height):
    rng = random.Random(17 * log_leaves + cap_height)
    check_tree(ctx, [kc.random_digest(rng) for _ in range(1 << log_leaves)], log_leaves, cap_height)


def test_two_wide_launches_level_by_level(ctx):
    log_leaves, cap_height = kc.TWO_WIDE_LEVEL_CASE
    rng = np.random.default_rng(15)
    dig = np.concatenate([rng.integers(0, 1 << 56, size=(1 << log_leaves, 3), dtype=np.uint64),
                          rng.integers(0, 1 << 32, size=(1 << log_leaves, 1), dtype=np.uint64)], axis=1)
    tree, cap = tree_of(ctx, dig, log_leaves, cap_height)
    assert (tree[:1 << log_leaves] == dig).all()
    at, n = 0, 1 << log_leaves
    for level in range(log_leaves - cap_height):
        below, here = tree[at:at + n], tree[at + n:at + n + n // 2]
        for i in kc.sampled_nodes(n // 2, 100 + level):
            want = kc.two_to_one([int(v) for v in below[2 * i]], [int(v) for v in below[2 * i + 1]])
            assert [int(v) for v in here[i]] == want, (level, i)
        at, n = at + n, n // 2
    assert n == 1 << cap_height and (tree[at:at + n] == cap).all()


def test_a_tree_of_all_ones_digests(ctx):
    log_leaves, cap_height = kc.ALL_ONES_LEVEL_CASE
    check_tree(ctx, [kc.ALL_ONES_DIGEST] * (1 << log_leaves), log_leaves, cap_height)


def test_levels_with_hasher_zero_are_the_poseidon_entry(ctx):
    import torch
    rng = random.Random(1)
    dig = [[rng.randrange(P) for _ in range(4)] for _ in range(1 << 9)]
    tree, cap = tree_of(ctx, dig, 9, ctx.cfg.cap_height, "poseidon")
    ref = torch.zeros((2 << 9, 4), dtype=torch.int64, device="cuda")
    ref[:1 << 9] = dev(np.array(dig, dtype=np.uint64))
    ref_cap = ctx.merkle_cap(ref, 9)
    assert (u64(ref) == tree).all() and (ref_cap == cap).all()


# ---- sipp_commit_batch_h --------------------------------------------------------------------------------------------------------------------
def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


@pytest.mark.parametrize("log_n, rate_bits, salted", [(4, 1, False), (4, 3, True), (10, 1, True), (10, 3, False)],
                         ids=["2^4_rate1", "2^4_rate3_salted", "2^10_rate1_salted", "2^10_rate3"])
def test_commit_batch_h_against_the_patched_reading(ctx, keccak_reading, log_n, rate_bits, salted):
    g = keccak_reading
    cap_height, n, m = 2, 1 << log_n, 1 << (log_n + rate_bits)
    ncols = 5 if log_n == 4 else 2                                            # (the reading's transforms are the slow part at 2^10)
    vals = rand_cols(log_n + rate_bits, ncols, n)
    salt = rand_cols(99, 4, m) if salted else None
    od, cap, keep = ctx.commit_ex(dev(vals), log_n, rate_bits, cap_height, salt=None if salt is None else dev(salt), hasher="keccak")
    batch = g.PolynomialBatch.from_values([[int(v) for v in col] for col in vals], rate_bits, 0 if salted else cap_height)
    if salted:        # the salt words follow the polynomials' in every leaf: natural LDE row r sits at leaf bitrev(r)
        leaves = [list(l) + [int(salt[q, bitrev(j, log_n + rate_bits)]) for q in range(4)] for j, l in enumerate(batch.tree.leaves)]
        want = g.MerkleTree(leaves, cap_height).cap
    else:
        want = batch.tree.cap
    assert [[int(v) for v in row] for row in cap] == want
    # hasher 0 through the new entry: sipp_commit_batch_ex word for word, tree and cap
    _, cap0, keep0 = ctx.commit_ex(dev(vals), log_n, rate_bits, cap_height, salt=None if salt is None else dev(salt), hasher="poseidon")
    _, cap1, keep1 = ctx.commit_ex(dev(vals), log_n, rate_bits, cap_height, salt=None if salt is None else dev(salt))
    top = 2 * m - (1 << cap_height)                                           # the nodes up to the cap level
    assert (cap0 == cap1).all() and (host(keep0[2])[:top] == host(keep1[2])[:top]).all() and (host(keep0[1]) == host(keep1[1])).all()


# ---- opening proofs ---------------------------------------------------------------------------------------------------------------------
FRI_ROWS = ("points-base7", "cap8_last_layer-11", "narrow-odd_salted", "no_rounds")       # smallest log_n; mixed arities with an arity-2
# round (hashed under Keccak, a no-op under Poseidon); salted oracles with leaves of 1 .. 4 words and more; no layer tree at all


def gpu_challenger_of(och):
    import sipp_amd
    return sipp_amd.Challenger.from_buffer_copy(bytes(och))


@pytest.mark.parametrize("row", FRI_ROWS)
def test_opening_proofs_under_keccak(ctx, keccak_reading, row):
    from sipp_amd import _lib
    g = keccak_reading
    case = fc.BY_ID[row]
    inst = fc.build(case)
    params = to_params(inst.fp)
    devs, caps, keep, devs0 = [], [], [], []
    for data, from_coeffs, salt in fc.device_inputs(inst):
        args = (dev(data), inst.log_n, inst.fp.rate_bits, inst.fp.cap_height)
        kw = dict(from_coeffs=from_coeffs, salt=None if salt is None else dev(salt))
        od, cap, bufs = ctx.commit_ex(*args, hasher="keccak", **kw)
        od0, cap0, bufs0 = ctx.commit_ex(*args, **kw)
        devs.append(od), caps.append(cap), keep.append((bufs, bufs0)), devs0.append(od0)
    start = bytes(fc.challenger(case))
    gch = gpu_challenger_of(start)
    proof = ctx.fri_prove_openings(devs, inst.batches, inst.log_n, params, gch, hasher="keccak")
    vch = gpu_challenger_of(start)
    assert _lib.fri_verify_openings_h(proof, caps, inst.ncols, inst.n_salt, inst.batches, inst.log_n, params, vch, "keccak") == 0
    assert bytes(vch) == bytes(gch)                                              # prover and verifier leave the transcript alike
    assert _lib.fri_verify_openings_h(proof, caps, inst.ncols, inst.n_salt, inst.batches, inst.log_n, params, gpu_challenger_of(start),
                                      "poseidon") in (123, 132)                  # the other hasher: a Merkle stage
    # EVERY query's paths again in the patched reading: the initial oracles' leaves to their caps, then round by round the layer tree's
    # leaf (the 2 << arity_bits evaluation words, hashed also at arity 2) at index x >> sum(arity_bits) to the round's cap in the proof
    log_m = inst.log_n + inst.fp.rate_bits
    ns0 = log_m - inst.fp.cap_height
    arities = [inst.fp.arity_bits[i] for i in range(inst.fp.n_rounds)]
    capw = 4 << inst.fp.cap_height
    qwords, lt = sum(inst.ncols) + sum(inst.n_salt) + 4 * ns0 * len(devs), log_m
    for a in arities:
        lt -= a
        qwords += (2 << a) + 4 * max(lt - inst.fp.cap_height, 0)
    q0 = inst.witness_index() + 1
    assert len(proof) == q0 + inst.fp.num_queries * qwords
    pf = [int(v) for v in proof]
    caps_at = q0 - 1 - 2 * ((1 << inst.log_n) >> sum(arities)) - len(arities) * capw
    round_caps = [[pf[caps_at + capw * r + 4 * i:caps_at + capw * r + 4 * i + 4] for i in range(capw // 4)] for r in range(len(arities))]
    lde0 = u64(keep[0][0][1])
    climbed = 0
    for qi in range(inst.fp.num_queries):
        at = q0 + qi * qwords
        # the index is not in the proof: it is the position of oracle 0's opened row (salt included) in that oracle's LDE
        leaf0 = np.array(pf[at:at + inst.ncols[0] + inst.n_salt[0]], dtype=np.uint64)
        hits = np.flatnonzero((lde0 == leaf0[:, None]).all(axis=0))
        assert len(hits) == 1
        x = int(hits[0])
        for o in range(len(devs)):
            ll = inst.ncols[o] + inst.n_salt[o]
            leaf = pf[at:at + ll]
            sib = [pf[at + ll + 4 * l:at + ll + 4 * l + 4] for l in range(ns0)]
            cap = [[int(v) for v in r] for r in caps[o]]
            assert g.verify_merkle_proof_to_cap(leaf, x, cap, sib), (qi, o)
            at += ll + 4 * ns0
        rounds, end = kc.layer_rounds(pf, at, x, arities, log_m, inst.fp.cap_height)
        assert end == q0 + (qi + 1) * qwords
        for r, (ev, xi, sib, _) in enumerate(rounds):
            assert g.verify_merkle_proof_to_cap(ev, xi, round_caps[r], sib), (qi, "round", r)
            climbed += 1
    assert climbed == inst.fp.num_queries * len(arities)
    # hasher 0 through the new entry: sipp_fri_prove_openings word for word
    a, b = gpu_challenger_of(start), gpu_challenger_of(start)
    p0 = ctx.fri_prove_openings(devs0, inst.batches, inst.log_n, params, a, hasher="poseidon")
    p1 = ctx.fri_prove_openings(devs0, inst.batches, inst.log_n, params, b)
    assert len(p0) == len(p1) and (p0 == p1).all() and bytes(a) == bytes(b)
    assert len(p0) == len(proof)                                                # proof sizes do not depend on the hasher


# ---- whole outer proofs ---------------------------------------------------------------------------------------------------------------------
class Outer:
    """the blinding catalogue's circuit (log_n = 10) through CircuitProver under one hasher"""

    def __init__(self, ctx, lookups, blinded, hasher):
        import sipp_amd
        from sipp_amd.circuit import CircuitProver
        self.c = c = bc.circuit(lookups, blind=blinded)
        self.gp = sipp_amd.PlonkParams(c.num_routed, D, NC)
        self.pr = CircuitProver(ctx, c, fri=bc.proof_fri(c.log_n, 0), params=self.gp, digest=bc.PROOF_DIGEST, zero_knowledge=blinded,
                                seed=bc.SEED if blinded else None, hasher=hasher)
        self.a, self.b = 9, 12
        self.y = c.value(self.a, self.b)
        self.circ = c.circuit()
        self.desc = tuple(self.circ.get("lookup", (0,) * 8))
        self.pc = sipp_amd.PlonkCircuit.from_dict(self.circ)

    def prove(self):
        return self.pr.prove(self.y, self.a, self.b)

    def reseed(self):
        if self.pr.fri.hiding:
            self.pr.data.set_blinding(bc.SEED)

    def verdict(self, proof, hasher):
        from sipp_amd import _lib
        return _lib.plonk_verify_gates_h(proof, self.pr.cap, self.gp, self.pr.fri, self.pc, bc.PROOF_DIGEST, self.desc if any(self.desc) else None,
                                         hasher)


KINDS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("lookups, blinded", KINDS, ids=["plain", "lookups", "blinded", "lookups_blinded"])
def test_whole_outer_proofs_under_keccak(ctx, lookups, blinded):
    from sipp_amd import _lib
    k = Outer(ctx, lookups, blinded, "keccak")
    p = Outer(ctx, lookups, blinded, "poseidon")
    try:
        proof = k.prove()
        assert int(proof[_lib.PLONK_HEADER_HASHER_WORD]) == 1 and int(proof[14]) == 0 and int(proof[15]) == 0
        assert k.pr.verify(proof) == (0, 0) and k.verdict(proof, "keccak") == 0
        assert k.verdict(proof, "poseidon") == 201
        hw = 24 if (lookups or blinded) else 16
        for o in range(3):            # digest words in their ranges, cap by cap
            cap = proof[hw + 64 * o:hw + 64 * (o + 1)].reshape(16, 4)
            assert (cap[:, :3] < np.uint64(1 << 56)).all() and (cap[:, 3] < np.uint64(1 << 32)).all()
        # equal (seed, counter): an equal proof; and the three prove paths of the circuit data agree word for word
        k.reseed()
        again = k.prove()
        assert len(again) == len(proof) and (again == proof).all()
        table = np.ascontiguousarray(k.c.partial_witness(k.y, k.a, k.b), dtype=np.uint64)
        cells = np.flatnonzero(table.reshape(-1)).astype(np.uint64)
        values = table.reshape(-1)[cells.astype(np.int64)]
        pis = k.c.public_inputs(k.y)
        k.reseed()
        by_cells = k.pr.data.prove_inputs(cells, values, pis)
        k.pr.data.set_input_map(cells, np.arange(len(cells), dtype=np.uint64), len(cells), 0)
        k.reseed()
        by_words = k.pr.data.prove_words(values, np.zeros(0, dtype=np.uint64), pis)
        assert (by_cells == proof).all() and (by_words == proof).all()
        # the Poseidon prover through the new build entry: today's proof, byte for byte; same length as the Keccak one
        ref = p.prove()
        import sipp_amd
        from sipp_amd.circuit import CircuitProver
        old = CircuitProver(ctx, p.c, fri=bc.proof_fri(p.c.log_n, 0), params=p.gp, digest=bc.PROOF_DIGEST, zero_knowledge=blinded,
                            seed=bc.SEED if blinded else None)
        try:
            built_h = sipp_amd.CircuitData(ctx, p.c.log_n, p.gp, p.pr.fri, p.pc, p.c.constants_sigmas(), p.c.generators(), sched=p.c.schedule(),
                                           digest=bc.PROOF_DIGEST, hasher="poseidon")
            try:
                if any(p.desc):
                    built_h.set_lookup(p.desc)
                if blinded:
                    built_h.set_blinding(bc.SEED)
                via_h = built_h.prove(p.c.partial_witness(p.y, p.a, p.b), pis)
            finally:
                built_h.close()
            want = old.prove(p.y, p.a, p.b)
        finally:
            old.close()
        assert int(ref[13]) == 0 and (ref == want).all() and (via_h == want).all() and len(ref) == len(proof)
        assert p.verdict(ref, "poseidon") == 0 and p.verdict(ref, "keccak") == 201
        # the recursion wrappers take Poseidon proofs only
        with pytest.raises(ValueError):
            _lib.refuse_keccak_proof(proof, "test")
    finally:
        k.pr.close()
        p.pr.close()


@pytest.mark.parametrize("lookups, blinded", KINDS, ids=["plain", "lookups", "blinded", "lookups_blinded"])
def test_the_wires_cap_of_a_keccak_proof_is_commit_batch_h_of_the_witness(ctx, lookups, blinded):
    """the direct entry, kind by kind: the witness is generated here, the proof's wires cap is sipp_commit_batch_h of those columns (with
    the reading's salt columns under blinding), and the verifier data is sipp_commit_batch_h of constants_sigmas"""
    import sipp_amd
    from sipp_amd import _lib
    c = bc.circuit(lookups, blind=blinded)
    circ = c.circuit()
    desc = tuple(circ["lookup"]) if lookups else None
    pc, gp, fp = sipp_amd.PlonkCircuit.from_dict(circ), sipp_amd.PlonkParams(c.num_routed, D, NC), bc.proof_fri(c.log_n, 1 if blinded else 0)
    blind = sipp_amd.Blinding.of(bc.SEED, 0) if blinded else None
    d_cs = dev(c.constants_sigmas())
    d_k = d_cs[:circ["num_constants"]]
    y = c.value(9, 12)
    pis = c.public_inputs(y)
    d_w = dev(c.partial_witness(y, 9, 12))
    pih = [int(x) for x in _oracle.hash_no_pad(pis)]
    ctx.plonk_generate_witness_levels(d_w, d_k, c.log_n, c.generators(), pih, sipp_amd.PlonkSchedule.from_dict(c.schedule()), blind=blind)
    if lookups:
        ctx.plonk_lookup_multiplicities(d_w, d_k, c.log_n, circ["num_selectors"], desc)
    proof = ctx.plonk_prove_gates_h(d_w, d_cs, c.log_n, gp, fp, pc, bc.PROOF_DIGEST, pis, desc, blind, "keccak")
    salt = dev(bc.salt_natural(bc.SEED, 0, bc.STREAM_WIRES, c.log_n + fp.rate_bits)) if blinded else None
    _, wires_cap, keep = ctx.commit_ex(d_w, c.log_n, fp.rate_bits, fp.cap_height, salt=salt, hasher="keccak")
    _, cs_cap, keep2 = ctx.commit_ex(d_cs, c.log_n, fp.rate_bits, fp.cap_height, hasher="keccak")
    hw = 24 if (lookups or blinded) else 16
    assert int(proof[13]) == 1 and (proof[hw:hw + 64] == wires_cap.reshape(-1)).all()
    assert _lib.plonk_verify_gates_h(proof, cs_cap, gp, fp, pc, bc.PROOF_DIGEST, desc, "keccak") == 0
    # hasher 0 through the new entry: the older entry of that kind, byte for byte
    via_h = ctx.plonk_prove_gates_h(d_w, d_cs, c.log_n, gp, fp, pc, bc.PROOF_DIGEST, pis, desc, blind, "poseidon")
    if blinded or lookups:
        old = ctx.plonk_prove_gates_zk(d_w, d_cs, c.log_n, gp, fp, pc, bc.PROOF_DIGEST, pis, desc if lookups else (0,) * 8, blind)
    else:
        old = ctx.plonk_prove_gates(d_w, d_cs, c.log_n, gp, fp, pc, bc.PROOF_DIGEST, pis)
    assert len(via_h) == len(old) == len(proof) and (via_h == old).all()


# ---- refusals, each followed by a good call on the same ctx ---------------------------------------------------------------------------------
def test_hasher_two_is_refused_everywhere(ctx):
    import sipp_amd
    from sipp_amd import _lib
    from sipp_amd.circuit import CircuitProver
    lde = dev(rand_cols(1, 5, 16))

    def refused(fn):
        with pytest.raises(sipp_amd.SippError) as err:
            fn()
        assert err.value.code == E_BADARG

    refused(lambda: ctx.merkle_leaves_h(lde, 4, 2))
    assert [int(v) for v in u64(ctx.merkle_leaves_h(lde, 4, "keccak"))[3]] == kc.hash_or_noop(int(v) for v in host(lde).astype(np.uint64)[:, 3])
    refused(lambda: ctx.fri_leaves_h(lde[:2], 1, 2))
    refused(lambda: tree_of(ctx, [kc.ALL_ONES_DIGEST] * 4, 2, 0, 2))
    check_tree(ctx, [kc.ALL_ONES_DIGEST] * 4, 2, 0)
    refused(lambda: ctx.commit_ex(dev(rand_cols(2, 2, 16)), 4, 1, 0, hasher=2))
    ctx.commit_ex(dev(rand_cols(2, 2, 16)), 4, 1, 0, hasher=1)
    case = fc.BY_ID["no_rounds"]
    inst = fc.build(case)
    devs, keep = [], []
    for data, from_coeffs, salt in fc.device_inputs(inst):
        od, cap, bufs = ctx.commit_ex(dev(data), inst.log_n, inst.fp.rate_bits, inst.fp.cap_height, from_coeffs=from_coeffs,
                                      salt=None if salt is None else dev(salt), hasher="keccak")
        devs.append(od), keep.append(bufs)
    start = bytes(fc.challenger(case))
    refused(lambda: ctx.fri_prove_openings(devs, inst.batches, inst.log_n, to_params(inst.fp), gpu_challenger_of(start), hasher=2))
    good = ctx.fri_prove_openings(devs, inst.batches, inst.log_n, to_params(inst.fp), gpu_challenger_of(start), hasher="keccak")
    with pytest.raises(sipp_amd.SippError):
        _lib.fri_verify_openings_h(good, [np.zeros(64, dtype=np.uint64)] * len(devs), inst.ncols, inst.n_salt, inst.batches, inst.log_n,
                                   to_params(inst.fp), gpu_challenger_of(start), 2)
    c = bc.circuit(False, blind=False)
    gp = sipp_amd.PlonkParams(c.num_routed, D, NC)
    pc = sipp_amd.PlonkCircuit.from_dict(c.circuit())
    refused(lambda: sipp_amd.CircuitData(ctx, c.log_n, gp, bc.proof_fri(c.log_n, 0), pc, c.constants_sigmas(), c.generators(), sched=c.schedule(),
                                         digest=bc.PROOF_DIGEST, hasher=2))
    with pytest.raises(ValueError):
        CircuitProver(ctx, c, fri=bc.proof_fri(c.log_n, 0), params=gp, digest=bc.PROOF_DIGEST, hasher="sha3")
    pr = CircuitProver(ctx, c, fri=bc.proof_fri(c.log_n, 0), params=gp, digest=bc.PROOF_DIGEST, hasher="keccak")
    try:
        y = c.value(9, 12)
        proof = pr.prove(y, 9, 12)
        assert pr.verify(proof) == (0, 0)
        d_cs, d_w = dev(c.constants_sigmas()), dev(c.partial_witness(y, 9, 12))
        refused(lambda: ctx.plonk_prove_gates_h(d_w, d_cs, c.log_n, gp, bc.proof_fri(c.log_n, 0), pc, bc.PROOF_DIGEST, c.public_inputs(y), None, None, 2))
        assert (pr.prove(y, 9, 12) == proof).all()
    finally:
        pr.close()


def test_the_recursion_provers_refuse_a_keccak_proof_before_anything_is_launched():
    """PlonkVerifierProver / FriProofProver.prove_proof: ValueError from the header word, before the circuit data is touched (none exists here)"""
    from sipp_amd.fri_proof import FriProofProver
    from sipp_amd.plonk_verifier import PlonkVerifierProver
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keccak_proof_small.npz"))
    for cls, args in ((PlonkVerifierProver, (z["proof"], z["cap"], bc.PROOF_DIGEST)), (FriProofProver, (z["proof"], [], [], ([0] * 12, [])))):
        shell = cls.__new__(cls)                                                # no ctx, no circuit data: the refusal needs neither
        with pytest.raises(ValueError):
            shell.prove_proof(*args)
    shell = FriProofProver.__new__(FriProofProver)
    with pytest.raises(ValueError):
        shell.prove_proof(np.zeros(8, dtype=np.uint64), [], [], ([0] * 12, []), hasher="keccak")
