"""The shape of the three outer circuits, pinned: for the smallest shapes that reach every branch of the wiring, everything a circuit
hands to the prover -- the gate set, the generators, the constant columns, the row order, the levels and the schedule, the copies, the
copy cycles, the sigma rows, and the public inputs and the partial witness of a fixed input -- hashes to the digests of
tests/golden/outer_circuit_shapes.json (tools/outer_circuit_shapes.py, whose digests() this test calls).  Of MerkleOpeningCircuit the
partition of the cells into cycles is pinned, not the order of the cells along a cycle."""
import json
import os
import sys

import pytest

from sipp_amd import fri_fold as ff
from sipp_amd import fri_initial as fi
from sipp_amd import merkle as mk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import outer_circuit_shapes as shapes  # noqa: E402

P = 0xFFFFFFFF00000001
SHAPES = [("merkle", s) for s in ((16, 9, 4, 28),               # (leaf_len, height, cap_height, n_paths): the other tests' shape
                                  (3, 1, 1, 1),                 # no leaf-hash rows, the leaf padded with zero cells
                                  (9, 2, 5, 2),                 # two RandomAccess copies per row, a partly filled second leaf row
                                  (4, 3, 6, 1))]                # one copy per row, four rows
SHAPES += [("fold", s) for s in ((11, 4, 2, 4, 4),              # (log_m, arity_bits, n_rounds, final_len, n_queries): the other tests' two
                                 (11, 2, 3, 16, 4),
                                 (4, 1, 1, 1, 1),               # final_len = 1: no Horner rows, the coefficient's cell is `old`
                                 (5, 2, 2, 2, 2))]
SHAPES += [("initial", s) for s in ((11, 5, [[0, 1, 2, 3, 4], [1, 3, 4]], 4, 2, 2),         # (log_m, n_columns, batches, n_queries, k_base, k_ext)
                                    (11, 5, [[0, 1, 2, 3, 4], [1, 3, 4]], 4, None, None),   # the default K: (25, 19)
                                    (3, 1, [[0]], 1, 1, 1),                                 # a batch of one: no power rows, no padding
                                    (4, 6, [[5, 0, 2, 2, 1, 3, 4], [4]], 2, 3, 2))]         # a repeated column, both chains with remainders


def name(kind, shape):
    return "%s%r" % (kind, tuple(shape))


def values(n, at):
    """n field values from position `at` of the fixed sequence p - 1, 0, 2, p - 1, 0, 5, ..."""
    return [(P - 1, 0, i)[i % 3] for i in range(at, at + n)]


def pairs(n, at):
    v = values(2 * n, at)
    return [(v[2 * i], v[2 * i + 1]) for i in range(n)]


def indices(n, bits):
    """the largest index, the one with only the top bit set, 0, then small ones"""
    return [((1 << bits) - 1, 1 << (bits - 1), 0, i % (1 << bits))[min(i, 3)] for i in range(n)]


def shape_digests(kind, shape):
    if kind == "merkle":
        leaf_len, height, cap_height, n_paths = shape
        c = mk.MerkleOpeningCircuit(*shape)
        public = (values(4 << cap_height, 0), indices(n_paths, cap_height + height), values(n_paths * leaf_len, 1))
        return shapes.digests(c, public + (values(n_paths * height * 4, 2),), public, sigma_rows=False)
    if kind == "fold":
        log_m, arity_bits, n_rounds, final_len, n_queries = shape
        c = ff.FriFoldCircuit(*shape)
        queries = [(x, pairs(1, q)[0], [pairs(1 << arity_bits, q + r) for r in range(n_rounds)]) for q, x in enumerate(indices(n_queries, log_m))]
        args = (pairs(n_rounds, 0), pairs(final_len, 1), queries)
        return shapes.digests(c, args, args)
    log_m, n_columns, batches, n_queries, k_base, k_ext = shape
    c = fi.FriInitialCircuit(log_m, n_columns, batches, n_queries, k_base=k_base, k_ext=k_ext)
    queries = [(x, values(n_columns, q), pairs(1, q + 1)[0]) for q, x in enumerate(indices(n_queries, log_m))]
    args = (pairs(1, 0)[0], pairs(len(batches), 1), [pairs(len(b), 2 + k) for k, b in enumerate(batches)], queries)
    return shapes.digests(c, args, args)


@pytest.mark.parametrize("kind,shape", SHAPES, ids=[name(*s) for s in SHAPES])
def test_shape_is_the_pinned_one(kind, shape):
    want = json.load(open(shapes.PATH))[name(kind, shape)]
    got = shape_digests(kind, shape)
    assert sorted(got) == sorted(want)
    assert [item for item in got if got[item] != want[item]] == []
