"""The Keccak-256 tree hasher without a GPU: the pure-Python reading (tests/_keccak_cases.py) at its known answers, the library's host
functions (sipp_host_keccak256, sipp_host_merkle_hash: what the verifier climbs paths with) against the reading, the stand-alone program
tests/host/keccak_check.cpp under AddressSanitizer + UBSan, and the committed proof tests/golden/keccak_proof_small.npz (captured on the
device by tools/capture_keccak_fixture.py): accepted, and refused stage by stage when damaged.

The hash, as read here and in DESIGN.md section 7: original Keccak-256 (rate 136, padding 0x01 .. 0x80); hash_no_pad = the canonical
elements as 8 little-endian bytes each, hashed, the first 25 bytes; hash_or_noop = up to three elements unhashed in a zeroed 25-byte array;
two_to_one = the hash of the 50 bytes l || r; a digest = four words of 7 + 7 + 7 + 4 bytes."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import sipp_amd
from sipp_amd import _lib
from tests import _blinding_cases as bc
from tests import _keccak_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = kc.P
D, NC = 8, 2


# ---- the reading itself --------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_reading():
    assert kc.keccak256(b"").hex() == kc.KAT_EMPTY
    assert kc.keccak256(b"abc").hex() == kc.KAT_ABC


def test_the_noop_form_is_a_recut_not_a_copy():
    assert kc.hash_or_noop([1, 2, 3]) == [1, 2 << 8, 3 << 16, 0]
    assert kc.hash_or_noop([P - 1]) == [(P - 1) & ((1 << 56) - 1), (P - 1) >> 56, 0, 0]
    assert kc.hash_or_noop([P + 5, 0, 0]) == [5, 0, 0, 0]                      # canonical bytes
    assert kc.hash_or_noop([1, 2, 3, 4]) == kc.hash_no_pad([1, 2, 3, 4]) != [1, 2, 3, 4]
    d = kc.hash_no_pad(range(20))
    assert all(w < 1 << 56 for w in d[:3]) and d[3] < 1 << 32
    assert kc.digest_words(kc.digest_bytes(d)) == d


# ---- the library's host functions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", kc.BLOCK_EDGE_LENGTHS)
def test_host_keccak256_at_the_block_edges(length):
    msg = bytes((37 * i + length) & 0xff for i in range(length))
    assert _lib.host_keccak256(msg) == kc.keccak256(msg)


def test_host_keccak256_known_answers():
    assert _lib.host_keccak256(b"").hex() == kc.KAT_EMPTY and _lib.host_keccak256(b"abc").hex() == kc.KAT_ABC


@pytest.mark.parametrize("n", kc.HOST_ELEMENT_COUNTS)
def test_host_hash_or_noop_against_the_reading(n):
    rng = random.Random(100 + n)
    for e in (kc.random_elements(rng, n), [P - 1] * n, [P, P + 1, (1 << 64) - 1, 7][:n] + kc.random_elements(rng, max(0, n - 4))):
        assert [int(x) for x in _lib.host_merkle_hash("keccak", e)] == kc.hash_or_noop(e), (n, e)


def test_host_two_to_one_against_the_reading():
    rng = random.Random(7)
    ones = kc.ALL_ONES_DIGEST
    pairs = [(kc.random_digest(rng), kc.random_digest(rng)) for _ in range(4)] + [(ones, ones), (ones, [0, 0, 0, 0]), ([0, 0, 0, 0], ones)]
    for l, r in pairs:
        assert [int(x) for x in _lib.host_merkle_hash("keccak", l, r)] == kc.two_to_one(l, r)


def test_host_merkle_hash_with_hasher_zero_is_poseidon_and_two_is_refused():
    from oracle.py import plonky2_generic as g
    e = list(range(1, 10))
    assert [int(x) for x in _lib.host_merkle_hash("poseidon", e)] == g.hash_or_noop(e)
    assert [int(x) for x in _lib.host_merkle_hash("poseidon", [1, 2, 3])] == [1, 2, 3, 0]
    assert [int(x) for x in _lib.host_merkle_hash("poseidon", [1, 2, 3, 4], [5, 6, 7, 8])] == g.two_to_one([1, 2, 3, 4], [5, 6, 7, 8])
    with pytest.raises(sipp_amd.SippError):
        _lib.host_merkle_hash(2, e)
    with pytest.raises(ValueError):
        _lib.hasher_id("sha3")


# ---- the stand-alone program under sanitizers ------------------------------------------------------------------------------------------
def _cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return c
    pytest.fail("no C++ compiler for the host test")


def test_host_keccak_header_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "keccak_check")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sipp_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "keccak_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "keccak_check ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]


# ---- the patched generic reading --------------------------------------------------------------------------------------------------------
@pytest.fixture
def keccak_reading(monkeypatch):
    """oracle/py/plonky2_generic.py with its two tree functions replaced: MerkleTree, verify_merkle_proof_to_cap, PolynomialBatch and
    fri_committed_trees look them up at call time; its Challenger keeps Poseidon (a challenge drawn before and after is the same)"""
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


def test_the_patched_reading_builds_keccak_trees(keccak_reading):
    g = keccak_reading
    rng = random.Random(3)
    leaves = [kc.random_elements(rng, 5) for _ in range(8)]
    t = g.MerkleTree(leaves, 1)
    assert t.levels == kc.merkle_levels([kc.hash_or_noop(l) for l in leaves], 1)
    assert g.verify_merkle_proof_to_cap(leaves[5], 5, t.cap, t.prove(5))


# ---- the committed proof ------------------------------------------------------------------------------------------------------------------
class Fixture:
    def __init__(self):
        z = np.load(os.path.join(ROOT, "tests", "golden", "keccak_proof_small.npz"))
        self.proof, self.cap = z["proof"], z["cap"]
        assert tuple(int(x) for x in z["seed"]) == bc.SEED
        self.c = bc.circuit(True)
        self.a, self.b = (int(x) for x in z["inputs"])
        self.circ = self.c.circuit()
        self.desc = tuple(self.circ["lookup"])
        self.pc = sipp_amd.PlonkCircuit.from_dict(self.circ)
        self.gp = sipp_amd.PlonkParams(self.c.num_routed, D, NC)
        self.fp = bc.proof_fri(10, 1)
        self.proof.setflags(write=False)
        # where the query rounds' leaves sit: the blinding catalogue's walk of a "SIPPPLK5" proof, which knows header word 13 as zero
        plain = self.proof.copy()
        plain[_lib.PLONK_HEADER_HASHER_WORD] = 0
        self.rounds = bc.query_rounds(plain, self.circ, bc.PROOF_DIGEST, self.fp, D, NC, 1)
        self.ns0 = 10 + self.fp.rate_bits - self.fp.cap_height
        # the FRI layer part of every round, and the rounds' caps (behind the section's header and its opened values)
        sec = bc.parse5(plain, self.circ, self.fp, D, NC, 1)
        self.arities = [self.fp.arity_bits[r] for r in range(self.fp.n_rounds)]
        self.capw = 4 << self.fp.cap_height
        self.round_caps_at = sec["section_at"] + 8 + 2 * sec["n_open"]
        self.layers = []
        for x, leaves, where in self.rounds:
            at = where[3] + len(leaves[3]) + 4 * self.ns0
            self.layers.append(kc.layer_rounds(self.proof, at, x, self.arities, 10 + self.fp.rate_bits, self.fp.cap_height)[0])

    def verdict(self, proof, hasher="keccak"):
        return _lib.plonk_verify_gates_h(proof, self.cap, self.gp, self.fp, self.pc, bc.PROOF_DIGEST, self.desc, hasher)

    def caps(self, proof):
        n = 4 << self.fp.cap_height
        return [[int(v) for v in self.cap.reshape(-1)]] + [[int(v) for v in proof[24 + n * o:24 + n * (o + 1)]] for o in range(3)]


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_the_fixture_is_accepted_and_names_its_hasher(fx):
    p = fx.proof
    assert int(p[0]) == bc.MAGIC5 and int(p[1]) == 10 and int(p[12]) == 1 and int(p[13]) == 1 and int(p[14]) == 0 and int(p[15]) == 0
    assert _lib.plonk_proof_hasher(p) == _lib.HASH_KECCAK25
    assert len(p) * 8 < 64 << 10 and int(p[-1]) == fx.c.value(fx.a, fx.b)
    assert fx.verdict(p) == 0


def test_the_fixtures_paths_climb_to_their_caps_in_the_patched_reading(fx, keccak_reading):
    g = keccak_reading
    caps = fx.caps(fx.proof)
    assert len(fx.rounds) == 2
    for x, leaves, where in fx.rounds:
        for o in range(4):
            at = where[o] + len(leaves[o])
            sib = [[int(v) for v in fx.proof[at + 4 * l:at + 4 * l + 4]] for l in range(fx.ns0)]
            cap = [caps[o][4 * i:4 * i + 4] for i in range(1 << fx.fp.cap_height)]
            assert g.verify_merkle_proof_to_cap(leaves[o], x, cap, sib), (x, o)


def test_the_fixtures_layer_paths_climb_to_the_round_caps_in_the_patched_reading(fx, keccak_reading):
    """the three arity-4 rounds of both queries: hash_or_noop of the eight evaluation words at index x >> (2, 4, 6), through the siblings,
    to the round's cap as the proof carries it"""
    g = keccak_reading
    assert fx.arities == [2, 2, 2] and len(fx.layers) == 2
    for q, rounds in enumerate(fx.layers):
        assert [len(sib) for _, _, sib, _ in rounds] == [7, 5, 3]
        for r, (ev, xi, sib, _) in enumerate(rounds):
            at = fx.round_caps_at + fx.capw * r
            cap = [[int(v) for v in fx.proof[at + 4 * i:at + 4 * i + 4]] for i in range(fx.capw // 4)]
            assert len(ev) == 8 and g.verify_merkle_proof_to_cap(ev, xi, cap, sib), (q, r)


def test_a_changed_layer_sibling_or_round_cap_word_is_refused_at_the_layers_merkle_stage(fx):
    for r in range(3):
        bad = fx.proof.copy()
        bad[fx.layers[1][r][3] + 4 + 2] ^= np.uint64(1)                        # word 2 of the round's second sibling
        assert fx.verdict(bad) == 132


@pytest.mark.parametrize("q, r, sibling", [(0, 0, 6), (0, 1, 0), (1, 2, 2)])
def test_a_layer_sibling_word_with_a_bit_above_its_range_is_stage_141(fx, q, r, sibling):
    """the verifier's range pass walks the layer part of every round too: the LAST sibling of a round, the first of the next, and the
    last round's last -- a walk that drifted by a word would check the wrong range (word 3 holds four bytes) or miss the word"""
    at = fx.layers[q][r][3] + 4 * sibling
    for word, bit in ((0, 56), (2, 60), (3, 32)):
        bad = fx.proof.copy()
        bad[at + word] |= np.uint64(1 << bit)
        assert fx.verdict(bad) == 141, (word, bit)
    ok = fx.proof.copy()
    ok[at + 3] ^= np.uint64(1 << 31)                                           # inside word 3's range: the path's own stage, not 141
    assert fx.verdict(ok) == 132


@pytest.mark.parametrize("r", [0, 1, 2])
def test_a_round_cap_word_with_a_bit_above_its_range_is_stage_141(fx, r):
    for digest, word, bit in ((0, 0, 56), (15, 3, 32), (7, 1, 63)):
        bad = fx.proof.copy()
        bad[fx.round_caps_at + fx.capw * r + 4 * digest + word] |= np.uint64(1 << bit)
        assert fx.verdict(bad) == 141, (digest, word, bit)


def test_a_changed_sibling_word_is_refused_at_its_merkle_stage(fx):
    x, leaves, where = fx.rounds[1]
    for o in range(4):
        bad = fx.proof.copy()
        bad[where[o] + len(leaves[o]) + 4 * 2 + 1] ^= np.uint64(1)             # word 1 of the third sibling: stays inside its range
        assert fx.verdict(bad) == 123 + min(o, 3)


def test_a_changed_cap_word_is_refused_by_the_vanishing_check_or_before(fx):
    for o in range(3):
        bad = fx.proof.copy()
        bad[24 + (4 << fx.fp.cap_height) * o + 5] ^= np.uint64(1)
        assert 0 < fx.verdict(bad) <= 210


@pytest.mark.parametrize("bit", [56, 63])
def test_a_sibling_word_with_a_bit_above_its_range_is_stage_141(fx, bit):
    x, leaves, where = fx.rounds[0]
    for o, word in ((0, 0), (3, 2)):
        bad = fx.proof.copy()
        bad[where[o] + len(leaves[o]) + word] |= np.uint64(1 << bit)
        assert fx.verdict(bad) == 141
    bad = fx.proof.copy()
    bad[where[1] + len(leaves[1]) + 3] |= np.uint64(1 << 32)                    # word 3 holds four bytes
    assert fx.verdict(bad) == 141


def test_a_cap_word_with_a_bit_above_its_range_is_stage_141(fx):
    n = 4 << fx.fp.cap_height
    for o in range(3):
        bad = fx.proof.copy()
        bad[24 + n * o + 4] |= np.uint64(1 << 56)
        assert fx.verdict(bad) == 141
        bad = fx.proof.copy()
        bad[24 + n * o + 7] |= np.uint64(1 << 32)
        assert fx.verdict(bad) == 141
    cap = fx.cap.copy().reshape(-1)
    cap[2] |= np.uint64(1 << 57)                                               # the verifier data's own cap
    assert _lib.plonk_verify_gates_h(fx.proof, cap, fx.gp, fx.fp, fx.pc, bc.PROOF_DIGEST, fx.desc, "keccak") == 141


def test_the_hashers_do_not_verify_each_others_proofs(fx):
    assert fx.verdict(fx.proof, "poseidon") == 201
    assert sipp_amd.plonk_verify_gates_lookup(fx.proof, fx.cap, fx.gp, fx.fp, fx.pc, bc.PROOF_DIGEST, fx.desc) == 201
    z = np.load(os.path.join(ROOT, "tests", "golden", "blinding_proof_small.npz"))
    assert _lib.plonk_verify_gates_h(z["proof"], z["cap"], fx.gp, fx.fp, fx.pc, bc.PROOF_DIGEST, fx.desc, "poseidon") == 0
    assert _lib.plonk_verify_gates_h(z["proof"], z["cap"], fx.gp, fx.fp, fx.pc, bc.PROOF_DIGEST, fx.desc, "keccak") == 201
    forged = fx.proof.copy()
    forged[13] = 0                                                             # the header alone relabelled: the paths do not climb under Poseidon
    assert fx.verdict(forged, "poseidon") not in (0, 201)
    with pytest.raises(sipp_amd.SippError):
        fx.verdict(fx.proof, 2)


def test_the_recursion_wrappers_refuse_a_keccak_proof_before_anything_runs(fx):
    with pytest.raises(ValueError):
        _lib.refuse_keccak_proof(fx.proof, "test")
    _lib.refuse_keccak_proof(np.load(os.path.join(ROOT, "tests", "golden", "blinding_proof_small.npz"))["proof"], "test")
