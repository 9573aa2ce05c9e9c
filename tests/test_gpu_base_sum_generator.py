"""SIPP_GEN_BASE_SUM (kind 15: the limbs of a BaseSum row -> their sum, include/sipp_hip.h) on the device against its Python-integer
reading (tests/_challenger_reading.base_sum_row), on the launch paths of witness.hip: the row-local call; a level of exactly 16384 rows
(plonk_witness_level_kernel) beside one of 16383 (sixteen lanes per row); thin levels of 1 and 5 rows in circuits that also hold a
Poseidon row, once per sixteen-lane kernel and instantiation, where lane 0 runs the short families; and the refusals of its layout
check, by their code, each leaving the table untouched and the next good call served."""
import numpy as np
import pytest

from tests import _challenger_reading as cr
from tests import _witness_reading as rd
from tests._device import NO_GRAPH, dev, first_mismatch, host, levels

pytestmark = pytest.mark.gpu

P = cr.P
NUM_WIRES, OTHER = 135, 99
SHAPES = [(1, 1), (2, 32), (64, 1), (21, 3)]                    # (n_limbs, bits per limb): selector value 1 + index
GENS = [(cr.GEN_BASE_SUM, 0, 1 + k, nl, bits, 0, 0, 0) for k, (nl, bits) in enumerate(SHAPES)]
N_PATTERNS = 8


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 28)
    yield c
    c.close()


def limbs_of(pattern, n_limbs, bits, rng):
    """all zero; all one (64 one-bit limbs: 2^64 - 1, which wraps); p and p - 1 as digit patterns; limbs of p - 1 and of 2^64 - 1 (field
    values, not digits: the second is not even canonical); random digits; random 64-bit words"""
    mask = (1 << bits) - 1
    if pattern in (0, 1):
        return [pattern] * n_limbs
    if pattern in (2, 3):
        return [((P + 2 - pattern) >> (bits * l)) & mask for l in range(n_limbs)]
    if pattern in (4, 5):
        return [(P - 1, (1 << 64) - 1)[pattern - 4]] * n_limbs
    if pattern == 6:
        return [int(v) & mask for v in rng.integers(0, 1 << 63, n_limbs)]
    return [int(v) for v in rng.integers(0, 1 << 64, n_limbs, dtype=np.uint64)]


def table(log_n, seed, held=lambda r: r % 7 != 6):
    """(wires, constants, the reading's table with EVERY held row generated): row r holds shape r % 4 unless `held` says it is another
    gate's; its limbs follow pattern (r // 4) % 8; every other cell is random"""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    w = rng.integers(0, P, (NUM_WIRES, n), dtype=np.uint64)
    k = np.full((1, n), OTHER, dtype=np.uint64)
    want = None
    for r in range(n):
        nl, bits = SHAPES[r % 4]
        w[1:1 + nl, r] = np.array(limbs_of((r // 4) % N_PATTERNS, nl, bits, rng), dtype=np.uint64)
        if held(r):
            k[0, r] = 1 + r % 4
    want = w.copy()
    for r in np.flatnonzero(k[0] != OTHER):
        nl, bits = SHAPES[int(k[0, r]) - 1]
        row = [int(v) for v in w[:, r]]
        cr.base_sum_row(row, nl, bits)
        want[0, r] = row[0]
    return w, k, want


@pytest.fixture(scope="module")
def wide():
    return table(15, 1501)


def test_the_table_reaches_its_edges(wide):
    w, k, want = wide
    n = w.shape[1]
    rows = lambda shape, pattern: [r for r in range(n) if r % 4 == shape and (r // 4) % N_PATTERNS == pattern and k[0, r] != OTHER]
    r = rows(2, 1)[0]                                           # 64 ones: 2^64 - 1 = 2^32 - 2 mod p
    assert int(want[0, r]) == (1 << 32) - 2
    assert int(want[0, rows(2, 2)[0]]) == 0 and int(want[0, rows(2, 3)[0]]) == P - 1 and int(want[0, rows(1, 2)[0]]) == 0
    r = rows(3, 5)[0]                                           # 21 limbs of 2^64 - 1: the word is reduced, not masked
    assert int(w[1, r]) == (1 << 64) - 1 and int(want[0, r]) == ((1 << 32) - 2) * sum(1 << (3 * l) for l in range(21)) % P
    assert (want[1:] == w[1:]).all() and (want[0, k[0] == OTHER] == w[0, k[0] == OTHER]).all()
    assert all(rows(s, p) for s in range(4) for p in range(N_PATTERNS))


def test_row_local(ctx, wide):
    w, k, want = wide
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, dev(k), 15, GENS)
    ctx.sync()
    assert first_mismatch(host(d_w), want) is None


@pytest.mark.parametrize("route", [0, NO_GRAPH], ids=["graph", "launches"])
def test_a_level_of_16384_rows_and_one_of_16383(ctx, wide, route):
    """level 0 = rows 0 .. 16382 (one row short of the kernel switch: sixteen lanes per row), level 1 = rows 16384 .. 32767 (exactly
    16384: one lane per row); row 16383 is in no level and stays as it was"""
    import sipp_amd
    w, k, want = wide
    want = want.copy()
    want[:, 16383] = w[:, 16383]
    assert k[0, 16383] != OTHER
    sc = levels([np.arange(16383), np.arange(16384, 32768)])
    assert list(np.diff(sc["level_offsets"].astype(np.int64))) == [16383, 16384]
    L = sipp_amd.lib()
    try:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
        d_w = dev(w)
        ctx.plonk_generate_witness_levels(d_w, dev(k), 15, GENS, None, sipp_amd.PlonkSchedule.from_dict(sc))
        assert first_mismatch(host(d_w), want) is None
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


# generator lists that pick each sixteen-lane kernel: one plain Poseidon generator -> plonk_witness_level_coop_kernel; a swap generator
# -> plonk_witness_level_coop_rows_kernel<false, false>; an interpolation generator besides -> <true, false>; a ReducingExt generator
# besides -> <true, true>.  Row 12 holds the Poseidon-family generator (selector value 5); no row holds the others.
POSEIDON = (rd.GEN_POSEIDON, 0, 5, 0, 12, 24, 0, 0)
SWAP = (rd.GEN_POSEIDON_SWAP, 0, 5, 0, 12, 29, 24, 25)
THIN = {"coop": GENS + [POSEIDON], "coop_rows": GENS + [SWAP],
        "coop_rows_interp": GENS + [SWAP, (rd.GEN_COSET_INTERPOLATION, 0, 6, 4, 7, 7, 0, 0)],
        "coop_rows_reduce": GENS + [SWAP, (rd.GEN_REDUCING_EXT, 0, 7, 19, 7, 0, 0, 0)]}


@pytest.mark.parametrize("kernel", sorted(THIN))
def test_thin_levels_beside_a_poseidon_row(ctx, kernel):
    """levels of 1 and of 5 rows (one block of four rows and a second block with one): the base-sum rows run on lane 0 of their sixteen"""
    import sipp_amd
    w, k, _ = table(10, 1502, held=lambda r: True)
    k[0, 12] = 5
    w[24, 12] = 1                                               # the swap wire
    gens = THIN[kernel]
    sc = levels([[3], [10, 11, 12, 13, 14]])
    want = rd.replay(w, k, gens, None, sc)
    assert (want[0, [3, 10, 11, 13, 14]] != w[0, [3, 10, 11, 13, 14]]).all() and (want[12:24, 12] != w[12:24, 12]).all()
    assert (np.delete(want, [3, 10, 11, 12, 13, 14], axis=1) == np.delete(w, [3, 10, 11, 12, 13, 14], axis=1)).all()
    d_w = dev(w)
    ctx.plonk_generate_witness_levels(d_w, dev(k), 10, gens, None, sipp_amd.PlonkSchedule.from_dict(sc))
    assert first_mismatch(host(d_w), want) is None


REFUSED = {"65_bits": (NUM_WIRES, (65, 1)), "13_limbs_of_5_bits": (NUM_WIRES, (13, 5)), "bits_0": (NUM_WIRES, (4, 0)),
           "bits_33": (NUM_WIRES, (1, 33)), "limbs_past_the_table": (8, (8, 1))}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_layouts_leave_the_table_untouched_and_the_next_call_is_served(ctx, name):
    import sipp_amd
    num_wires, (nl, bits) = REFUSED[name]
    w, k, want = table(10, 1503)
    w, want = np.ascontiguousarray(w[:num_wires]), np.ascontiguousarray(want[:num_wires])
    bad = [(cr.GEN_BASE_SUM, 0, 1, nl, bits, 0, 0, 0)]
    good = [g for g in GENS if 1 + g[3] <= num_wires]
    for r in np.flatnonzero(k[0] != OTHER):                     # the narrow table: rows of a shape it cannot hold are another gate's
        if 1 + SHAPES[int(k[0, r]) - 1][0] > num_wires:
            want[0, r] = w[0, r]
            k[0, r] = OTHER
    sched = sipp_amd.PlonkSchedule.from_dict(levels([np.arange(1024)]))
    d_w, d_k = dev(w), dev(k)
    for call in (lambda g: ctx.plonk_generate_witness(d_w, d_k, 10, g), lambda g: ctx.plonk_generate_witness_levels(d_w, d_k, 10, g, None, sched)):
        with pytest.raises(sipp_amd.SippError) as e:
            call(good + bad)
        assert e.value.code == -1                               # SIPP_E_BADARG, as kind 2's limits
        ctx.sync()
        assert first_mismatch(host(d_w), w) is None
        call(good)
        ctx.sync()
        assert first_mismatch(host(d_w), want) is None
        d_w.copy_(dev(w))
