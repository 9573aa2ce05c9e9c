"""SIPP_GEN_POSEIDON_MDS (kind 16: the permutation's linear layer on twelve extension elements, include/sipp_hip.h) on the device against
its Python-integer reading (tests/_poseidon_mds_reading.mds_row), on the launch paths of witness.hip: the row-local call; a level of
exactly 16384 rows (plonk_witness_level_kernel) beside one of 16383 (sixteen lanes per row, the row on lane 0); thin levels of 1 and 5
rows in circuits that also hold a Poseidon row, once per sixteen-lane kernel and instantiation; and the refusals of its layout check,
by their code, each leaving the table untouched and the next good call served.  The table's inputs reach the edges of the exact
half-product sum -- the low sum's wrap and a carry out of the high sum, for every output -- which a test without a device asserts."""
import numpy as np
import pytest

from tests import _poseidon_mds_reading as pm
from tests import _witness_reading as rd
from tests._device import NO_GRAPH, dev, first_mismatch, host, levels

gpu = pytest.mark.gpu

P = pm.P
NUM_WIRES, OTHER = 135, 99
LAYOUTS = [(0, 24), (60, 10)]                                   # (in, out): selector value 1 + index
GENS = [(pm.GEN_POSEIDON_MDS, 0, 1 + k, in_, out, 0, 0, 0) for k, (in_, out) in enumerate(LAYOUTS)]
N_PATTERNS = 8
M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 28)
    yield c
    c.close()


def inputs_of(pattern, target, rng):
    """24 words, element c limb l at 2 c + l: all zero; all p - 1; all 2^64 - 1 (not canonical; the low sum lands just below 2^64
    and does NOT wrap); low halves only; high halves only; for output `target` a high sum just below 2^32 under full low halves, so
    that al + 2^32 ah wraps; full high halves, so that the high sum carries past 2^32 (for every output); random words"""
    if pattern in (0, 1, 2):
        return [(0, P - 1, (1 << 64) - 1)[pattern]] * 24
    if pattern == 3:
        return [int(v) for v in rng.integers(0, 1 << 32, 24, dtype=np.uint64)]
    if pattern == 4:
        return [int(v) << 32 for v in rng.integers(0, 1 << 32, 24, dtype=np.uint64)]
    if pattern == 5:
        return [((M32 // pm.M[target][target]) << 32 if c == target else 0) | M32 for c in range(12) for _ in range(2)]
    if pattern == 6:
        return [(M32 << 32) | int(v) for v in rng.integers(0, 1 << 32, 24, dtype=np.uint64)]
    return [int(v) for v in rng.integers(0, 1 << 64, 24, dtype=np.uint64)]


def table(log_n, seed, held=lambda r: r % 7 != 6):
    """(wires, constants, the reading's table with EVERY held row generated): row r holds layout r % 2 unless `held` says it is another
    gate's; its inputs follow pattern (r // 2) % 8 with target output (r // 16) % 12; every other cell is random"""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    w = rng.integers(0, P, (NUM_WIRES, n), dtype=np.uint64)
    k = np.full((1, n), OTHER, dtype=np.uint64)
    for r in range(n):
        in_, _ = LAYOUTS[r % 2]
        w[in_:in_ + 24, r] = np.array(inputs_of((r // 2) % N_PATTERNS, (r // 16) % 12, rng), dtype=np.uint64)
        if held(r):
            k[0, r] = 1 + r % 2
    want = w.copy()
    for r in np.flatnonzero(k[0] != OTHER):
        in_, out = LAYOUTS[int(k[0, r]) - 1]
        row = w[:, r].tolist()
        pm.mds_row(row, in_, out)
        want[out:out + 24, r] = np.array(row[out:out + 24], dtype=np.uint64)
    return w, k, want


@pytest.fixture(scope="module")
def wide():
    return table(15, 1601)


def test_the_table_reaches_its_edges(wide):
    """no device: the two predicates of the device's half-product sum in Python integers, for every output, layout and limb"""
    w, k, want = wide
    n = w.shape[1]
    wrap, carry, neither = set(), set(), set()
    for r in range(3 * 16 * 12 * 2):                            # every (layout, pattern, target) several times over
        if k[0, r] == OTHER:
            continue
        lay, pattern = r % 2, (r // 2) % N_PATTERNS
        in_, out = LAYOUTS[lay]
        for l in range(2):
            words = [int(w[in_ + 2 * c + l, r]) for c in range(12)]
            for o in range(12):
                al, ah, wraps, top = pm.half_sums(words, o)
                assert int(want[out + 2 * o + l, r]) == (al + (ah << 32)) % P
                if not wraps and not top:
                    neither.add((lay, l, o))
                if wraps:
                    wrap.add((lay, l, o))
                if top:
                    carry.add((lay, l, o))
                if pattern == 2:                                # all 2^64 - 1: carries, and stops S short of wrapping
                    assert top and not wraps and (al + ((ah << 32) % (1 << 64))) == (1 << 64) - sum(pm.M[o])
    every = {(lay, l, o) for lay in range(2) for l in range(2) for o in range(12)}
    assert wrap == every and carry == every and neither == every
    rows = lambda lay, pattern: [r for r in range(n) if r % 2 == lay and (r // 2) % N_PATTERNS == pattern and k[0, r] != OTHER]
    assert all(rows(lay, p) for lay in range(2) for p in range(N_PATTERNS))
    for lay, (in_, out) in enumerate(LAYOUTS):
        assert (want[out:out + 24, rows(lay, 0)[0]] == 0).all()
        r = rows(lay, 1)[0]                                     # all p - 1: out_r = -(sum of row r)
        assert [int(v) for v in want[out:out + 24:2, r]] == [P - sum(pm.M[o]) for o in range(12)]
        r = rows(lay, 2)[0]                                     # all 2^64 - 1 = 2^32 - 2 mod p: the word is reduced, not masked
        assert int(w[in_, r]) == (1 << 64) - 1 and int(want[out + 1, r]) == (M32 - 1) * sum(pm.M[0]) % P
    untouched = np.ones(w.shape, dtype=bool)
    for lay, (in_, out) in enumerate(LAYOUTS):
        untouched[out:out + 24, k[0] == 1 + lay] = False
    assert int(want[~untouched].max()) < P                      # the outputs are canonical
    assert (want[untouched] == w[untouched]).all() and (want[~untouched] != w[~untouched]).mean() > 0.99


@gpu
def test_row_local(ctx, wide):
    w, k, want = wide
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, dev(k), 15, GENS)
    ctx.sync()
    assert first_mismatch(host(d_w), want) is None


@gpu
@pytest.mark.parametrize("route", [0, NO_GRAPH], ids=["graph", "launches"])
def test_a_level_of_16384_rows_and_one_of_16383(ctx, wide, route):
    """level 0 = rows 0 .. 16382 (one row short of the kernel switch: sixteen lanes per row, the row on lane 0), level 1 = rows
    16384 .. 32767 (exactly 16384: one lane per row); row 16383 is in no level and stays as it was"""
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


@gpu
@pytest.mark.parametrize("kernel", sorted(THIN))
def test_thin_levels_beside_a_poseidon_row(ctx, kernel):
    """levels of 1 and of 5 rows (one block of four rows and a second block with one): the MDS rows run on lane 0 of their sixteen"""
    import sipp_amd
    w, k, _ = table(10, 1602, held=lambda r: True)
    k[0, 12] = 5
    w[:24, 12] = np.random.default_rng(1605).integers(0, P, 24, dtype=np.uint64)     # the Poseidon row's inputs: canonical
    w[24, 12] = 1                                               # the swap wire
    gens = THIN[kernel]
    sc = levels([[3], [10, 11, 12, 13, 14]])
    want = rd.replay(w, k, gens, None, sc)
    for r in (3, 10, 11, 13, 14):
        out = LAYOUTS[r % 2][1]
        assert (want[out:out + 24, r] != w[out:out + 24, r]).all()
    assert (want[12:24, 12] != w[12:24, 12]).all()
    assert (np.delete(want, [3, 10, 11, 12, 13, 14], axis=1) == np.delete(w, [3, 10, 11, 12, 13, 14], axis=1)).all()
    d_w = dev(w)
    ctx.plonk_generate_witness_levels(d_w, dev(k), 10, gens, None, sipp_amd.PlonkSchedule.from_dict(sc))
    assert first_mismatch(host(d_w), want) is None


# (in, out) on a table of NUM_WIRES wires
REFUSED = {"inputs_past_the_table": (NUM_WIRES - 23, 0), "outputs_past_the_table": (0, NUM_WIRES - 23), "overlapping_by_one": (23, 0),
           "overlapping_the_other_way": (0, 23), "the_same_range": (40, 40), "input_start_wraps_32_bits": (0xFFFFFFF0, 0)}


@gpu
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_layouts_leave_the_table_untouched_and_the_next_call_is_served(ctx, name):
    import sipp_amd
    in_, out = REFUSED[name]
    w, k, want = table(10, 1603)
    bad = [(pm.GEN_POSEIDON_MDS, 0, 1, in_, out, 0, 0, 0)]
    sched = sipp_amd.PlonkSchedule.from_dict(levels([np.arange(1024)]))
    d_w, d_k = dev(w), dev(k)
    for call in (lambda g: ctx.plonk_generate_witness(d_w, d_k, 10, g), lambda g: ctx.plonk_generate_witness_levels(d_w, d_k, 10, g, None, sched)):
        with pytest.raises(sipp_amd.SippError) as e:
            call(GENS + bad)
        assert e.value.code == -1                               # SIPP_E_BADARG
        ctx.sync()
        assert first_mismatch(host(d_w), w) is None
        call(GENS)
        ctx.sync()
        assert first_mismatch(host(d_w), want) is None
        d_w.copy_(dev(w))


@gpu
def test_touching_ranges_are_served(ctx):
    """in + 24 = out and out + 24 = in are no overlap; the last wire of the table may be an output"""
    w, k, _ = table(10, 1604)
    for in_, out in ((0, 24), (24, 0), (NUM_WIRES - 48, NUM_WIRES - 24)):
        gens = [(pm.GEN_POSEIDON_MDS, 0, 1, in_, out, 0, 0, 0)]
        want = rd.row_local(w, k, gens, None)
        d_w = dev(w)
        ctx.plonk_generate_witness(d_w, dev(k), 10, gens)
        ctx.sync()
        assert first_mismatch(host(d_w), want) is None and (want != w).any()
