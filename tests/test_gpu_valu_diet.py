"""The two-chain reduction of the lazy sums (gl.hpp reduce6: 22 per permutation in both leaf kernels, and in the quotient's linear forms)
through the kernels that run it, bit for bit against the CPU oracle, at the smallest sizes where each kernel and each route is taken.
The commitments also run the tree sweeps of ntt_tree.hip, whose butterflies are NOT changed here: those cases guard the sweeps for a later
attempt to move them to the hand-scheduled product (profiles/r07_valu_diet.txt).

Edge columns: all 0, all p - 1, all 2^32 - 1, all 2^32 (the carries between the 32-bit halves) next to random cells.  A batch of ONE
column has no room for a constant column next to a random one: there the four edge words sit on every seventh cell of the random column."""
import numpy as np
import pytest

from tests import _oracle
from tests._device import dev, host
from tests._oracle import P

pytestmark = pytest.mark.gpu

EDGE_COLUMNS = [0, P - 1, (1 << 32) - 1, 1 << 32]


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=2 << 30)
    yield c
    c.close()


def cells_with_edge_columns(rng, ncols, n):
    """random cells; the LAST columns (as many of the four as leave one random column) are constant edge columns, so that they fall into
    the ragged last chunk of the absorption as well as into whole ones"""
    a = _oracle.rand_field(rng, (ncols, n))
    k = min(len(EDGE_COLUMNS), ncols - 1)
    for i in range(k):
        a[ncols - k + i, :] = EDGE_COLUMNS[i]
    if k < len(EDGE_COLUMNS):                 # a single column: the edge words in turn on every seventh cell
        for i, w in enumerate(EDGE_COLUMNS):
            a[0, 7 * i + 3::28] = w
    return a


@pytest.mark.parametrize("n_leaves", [16, 32, 64])
@pytest.mark.parametrize("ncols", [5, 8, 9, 17])
def test_leaf_digests_small(ctx, ncols, n_leaves):
    """16 leaves: the one-state-per-lane kernel; 32 and 64: the two-lane kernel at its smallest; 5 / 9 / 17 columns leave a ragged last
    chunk of the rate-8 absorption, 8 a whole one -- every leaf against hash_n_to_hash_no_pad of the oracle"""
    rng = np.random.default_rng(7000 + 100 * ncols + n_leaves)
    cells = cells_with_edge_columns(rng, ncols, n_leaves)
    dig = host(ctx.poseidon_leaves(dev(cells), n_leaves.bit_length() - 1))
    for j in range(n_leaves):
        assert (dig[j] == _oracle.hash_no_pad(cells[:, j])).all(), (ncols, n_leaves, j)


def test_leaf_digests_fat_route(ctx):
    """2^17 leaves x 9 columns: past the two-lane kernel's range, the one-state-per-lane kernel with whole waves and blocks (its
    matrix-pipe form); the first and last leaves of the launch and every 509th in between"""
    log_leaves, ncols = 17, 9
    n = 1 << log_leaves
    rng = np.random.default_rng(7917)
    cells = cells_with_edge_columns(rng, ncols, n)
    dig = host(ctx.poseidon_leaves(dev(cells), log_leaves))
    for j in list(range(64)) + list(range(64, n - 64, 509)) + list(range(n - 64, n)):
        assert (dig[j] == _oracle.hash_no_pad(cells[:, j])).all(), j


@pytest.mark.parametrize("log_n", [13, 14, 16, 18])
@pytest.mark.parametrize("ncols", [1, 5])
def test_commitments(ctx, log_n, ncols):
    """2^13: the smallest size the tree sweeps take (gather, middle, contiguous forward); 2^14: the Fq12 trace's; 2^16: three sweeps with
    eight inverse levels in the middle one; 2^18: four, with a strided inverse sweep (ntt_tree_inv) -- coefficients, every LDE cell
    and the cap (leaf hashing and the Merkle levels over them) equal the oracle's.  Five columns: one random, four constant edge columns;
    one column: random cells with the edge words on every seventh"""
    rng = np.random.default_rng(7100 + 10 * log_n + ncols)
    vals = cells_with_edge_columns(rng, ncols, 1 << log_n)
    ref = _oracle.Batch(vals, log_n)
    coeffs, lde, tree, cap = ctx.commit(dev(vals), log_n)
    assert (host(coeffs) == ref.coeffs).all()
    assert (host(lde).T == ref.leaves).all()
    assert (cap == ref.cap).all()
