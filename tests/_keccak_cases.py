"""The reading of the Keccak-256 tree hasher (plonky2 hash/keccak.rs KeccakHash<25>, as recalled) in plain Python, and the catalogue of
shapes the device kernels are held to (tests/test_gpu_keccak.py, tests/test_keccak_reading.py).

  keccak256      original Keccak: rate 136 bytes, padding 0x01 .. 0x80 (hashlib.sha3_256 pads with 0x06 and is NOT this function)
  hash_no_pad    every element as its canonical u64, 8 bytes little endian, concatenated; keccak256; the first 25 bytes
  hash_or_noop   at most 3 elements: the 24 bytes in a zeroed 25-byte array, nothing hashed -- re-cut into 7-byte words, not a copy
  two_to_one     keccak256 of the 50 bytes l || r, the first 25 bytes
  a digest       four words: bytes 0..6, 7..13, 14..20, 21..24, little endian

About 0.5 ms per permutation here: the catalogue is sized by that."""
import random

P = 2**64 - 2**32 + 1
M64 = (1 << 64) - 1
RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
      0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
ROT = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]      # [x][y]


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f(a):
    """Keccak-f[1600] on a[x][y], in place"""
    for rc in RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rol(a[x][y], ROT[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & M64 & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def keccak256(data):
    data = bytes(data)
    pad = 136 - len(data) % 136
    msg = data + (b"\x81" if pad == 1 else b"\x01" + b"\x00" * (pad - 2) + b"\x80")
    a = [[0] * 5 for _ in range(5)]
    for off in range(0, len(msg), 136):
        for i in range(17):
            a[i % 5][i // 5] ^= int.from_bytes(msg[off + 8 * i: off + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def digest_words(b25):
    assert len(b25) == 25
    return [int.from_bytes(b25[0:7], "little"), int.from_bytes(b25[7:14], "little"), int.from_bytes(b25[14:21], "little"),
            int.from_bytes(b25[21:25], "little")]


def digest_bytes(words):
    w = [int(x) for x in words]
    assert all(x < 1 << 56 for x in w[:3]) and w[3] < 1 << 32, "a digest word outside its range"
    return w[0].to_bytes(7, "little") + w[1].to_bytes(7, "little") + w[2].to_bytes(7, "little") + w[3].to_bytes(4, "little")


def element_bytes(elements):
    return b"".join((int(e) % P).to_bytes(8, "little") for e in elements)


def hash_no_pad(elements):
    return digest_words(keccak256(element_bytes(elements))[:25])


def hash_or_noop(elements):
    elements = list(elements)
    if 8 * len(elements) <= 25:
        return digest_words(element_bytes(elements).ljust(25, b"\x00"))
    return hash_no_pad(elements)


def two_to_one(left, right):
    return digest_words(keccak256(digest_bytes(left) + digest_bytes(right))[:25])


def merkle_levels(leaf_digests, cap_height):
    """the levels of a tree from its leaf digests up to the cap (min(cap_height, log leaves)), level 0 first"""
    levels = [[list(d) for d in leaf_digests]]
    n = len(leaf_digests)
    ch = min(cap_height, n.bit_length() - 1)
    while len(levels[-1]) > (1 << ch):
        prev = levels[-1]
        levels.append([two_to_one(prev[2 * i], prev[2 * i + 1]) for i in range(len(prev) // 2)])
    return levels


# ---------------------------------------------------------------------------------------------------------------- the catalogue
KAT_EMPTY = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
KAT_ABC = "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
BLOCK_EDGE_LENGTHS = (0, 1, 135, 136, 137, 271, 272, 273)
HOST_ELEMENT_COUNTS = (1, 3, 4, 16, 17, 18)
ALL_ONES_DIGEST = [(1 << 56) - 1, (1 << 56) - 1, (1 << 56) - 1, (1 << 32) - 1]

# (log_leaves, ncols): 1 and 3 the no-op form, 4 the first hashed, 16 = 128 bytes, 17 = one full block (the padding falls into a second),
# 18 / 33 / 34 / 35 around two blocks, 137 = wires + salt; leaf counts 2^0, 2^4, 2^5 (one wave and less), 2^8 + (more than one block of
# 256 lanes), up to 2^13 x 5 (32 blocks)
LEAF_CASES = ((0, 1), (0, 17), (4, 3), (4, 4), (4, 34), (5, 16), (5, 18), (5, 137), (8, 17), (8, 33), (9, 35), (9, 1), (10, 18), (13, 5))
NONCANONICAL_CASE = (6, 19)
FRI_LEAF_CASES = tuple((log_leaves, ab) for ab in (1, 2, 3, 4) for log_leaves in (4, 9))
# (log_leaves, cap_height): every size 2^1 .. 2^11 (one block climbs to the cap), cap heights 0, 1, 4 and one above log_leaves; 2^12 and
# 2^13 leaves are where the level kernel's launches change shape (blocks of 2^11 nodes climb three levels, then one block the rest)
LEVEL_CASES = ((1, 0), (1, 4), (2, 1), (3, 0), (4, 4), (5, 1), (6, 0), (7, 4), (8, 1), (9, 0), (10, 4), (11, 1), (11, 0), (12, 0), (13, 1))
# the wide launch cut short by the cap: 2^13 leaves with cap height 12 (one level) and 11 (two levels); the whole reading of these is the
# 2^12 / 2^12 + 2^11 nodes above the leaves
SHORT_WIDE_LEVEL_CASES = ((13, 12), (13, 11))
# two wide launches in a row (2^15 -> 2^12 -> 2^9 nodes): the whole reading would be 32 k permutations, so every level is checked node by
# node against the level below it AS THE DEVICE WROTE IT -- the first and last node of every block of 2^11 children and 48 drawn from a
# fixed seed; level by level that pins the tree, given the leaf digests
TWO_WIDE_LEVEL_CASE = (15, 9)
ALL_ONES_LEVEL_CASE = (6, 1)


def sampled_nodes(n_parents, seed):
    """parents of one level that TWO_WIDE_LEVEL_CASE compares: the first and last parent of every block (2^10 parents) and 48 drawn"""
    picks = set()
    for b in range(0, n_parents, 1 << 10):
        picks.update((b, min(b + (1 << 10), n_parents) - 1))
    picks.update(random.Random(seed).sample(range(n_parents), min(48, n_parents)))
    return sorted(picks)


def layer_rounds(words, at, x, arities, log_m, cap_height):
    """the FRI layer part of one query round of an opening section, from word `at`, for the query index x: per round
    (the 2 << arity_bits evaluation words = the layer tree's leaf, the leaf's index, its siblings, where the siblings start);
    and the position behind the round"""
    out, lt, xi = [], log_m, x
    for ab in arities:
        lt -= ab
        xi >>= ab
        ns = max(lt - cap_height, 0)
        ev = [int(v) for v in words[at:at + (2 << ab)]]
        at += 2 << ab
        out.append((ev, xi, [[int(v) for v in words[at + 4 * l:at + 4 * l + 4]] for l in range(ns)], at))
        at += 4 * ns
    return out, at


def random_elements(rng, n):
    return [rng.randrange(P) for _ in range(n)]


def random_digest(rng):
    return [rng.randrange(1 << 56), rng.randrange(1 << 56), rng.randrange(1 << 56), rng.randrange(1 << 32)]


def checked_leaves(log_leaves, seed=2024):
    """the leaves a test compares: all of them below 2^10, else the first and last leaf of every 256-lane block and 64 drawn from a
    fixed seed"""
    n = 1 << log_leaves
    if log_leaves < 10:
        return list(range(n))
    picks = set()
    for b in range(0, n, 256):
        picks.update((b, b + 255))
    picks.update(random.Random(seed).sample(range(n), 64))
    return sorted(picks)
