"""Several tagged lookup tables and SIPP_GEN_LOOKUP on the device, against the exact Python-integer reading of
tests/_lookup_tables_cases.py.  Tags (sipp_amd/csrc/lookup.hip, description word 7): the multiplicities and the S / U columns word for
word for every entry of the catalogue; a pair that exists only under the other tag refused with SIPP_E_WITNESS and accepted with
word 7 = 0; the refusals of word 7; a whole proof through the library's verifier and the reading.  Generator (witness.hip): every
instance cell for cell on sipp_plonk_generate_witness and on sipp_plonk_generate_witness_levels, whose thin levels run on either
sixteen-lane kernel and whose 16384-row level on the one-lane kernel, at both widths of the argument struct, through the captured
graph, its replay and launch by launch; the layout refusals.  Whole circuit (tests/_lookup_tables_circuit.py): two tables, an
arithmetic row, a function lookup and an in-circuit public-input hash on the three prove paths."""
import ctypes as C

import numpy as np
import pytest

from tests import _lookup_cases as lc
from tests import _lookup_tables_cases as tc
from tests._device import NO_GRAPH, dev, host

pytestmark = pytest.mark.gpu
POSEIDON_SWAP = 9                    # include/sipp_hip.h SIPP_GEN_POSEIDON_SWAP


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def device_multiplicities(ctx, e, desc=None):
    return host(ctx.plonk_lookup_multiplicities(dev(e["wires"]), dev(e["consts"]), e["log_n"], e["num_selectors"], desc or e["desc"]))


def device_sums(ctx, e, wires):
    import sipp_amd
    gp = sipp_amd.PlonkParams(1, e["D"], e["C"])
    return host(ctx.plonk_lookup_sums(dev(wires), dev(e["consts"]), e["log_n"], e["num_selectors"], gp, e["desc"], e["etas"], e["thetas"]))


def good_call(ctx):
    e = tc.BY_NAME[tc.GOOD_AFTER_REFUSAL]()
    want = tc.multiplicities(e["desc"], e["wires"], e["consts"])
    msg = tc.first_mismatch(device_multiplicities(ctx, e), want)
    assert msg is None, "after the refusal: " + msg
    cols, _ = tc.sums(e["desc"], want, e["consts"], e["D"], e["etas"], e["thetas"])
    msg = tc.first_mismatch(device_sums(ctx, e, want), cols)
    assert msg is None, "after the refusal: " + msg


# ---- tags -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.IDS)
def test_tagged_multiplicities_and_sums_are_the_readings(ctx, name):
    """every wire cell after the multiplicities (a pair under both tags is counted under each: the counts split by tag), then every
    S / U cell from the device's own multiplicities"""
    e = tc.BY_NAME[name]()
    want = tc.multiplicities(e["desc"], e["wires"], e["consts"])
    got = device_multiplicities(ctx, e)
    msg = tc.first_mismatch(got, want)
    assert msg is None, msg
    cols, closes = tc.sums(e["desc"], want, e["consts"], e["D"], e["etas"], e["thetas"])
    assert closes
    msg = tc.first_mismatch(device_sums(ctx, e, got), cols)
    assert msg is None, msg


@pytest.mark.parametrize("name", [f.__name__ for f in tc.SPOILED])
def test_a_pair_only_under_the_other_tag_is_refused_and_word_7_is_why(ctx, setup, name):
    import sipp_amd
    e = tc.BY_NAME[name]()
    with pytest.raises(tc.Absent):
        tc.multiplicities(e["desc"], e["wires"], e["consts"])
    with pytest.raises(sipp_amd.SippError) as err:
        device_multiplicities(ctx, e)
    assert err.value.code == tc.E_WITNESS
    # the same instance as ONE table: every looked-up pair is in some table slot
    one = e["desc"][:7] + (0,)
    msg = tc.first_mismatch(device_multiplicities(ctx, e, one), lc.multiplicities(one, e["wires"], e["consts"]))
    assert msg is None, msg
    good_call(ctx)
    proof = setup.raw(ctx, setup.wires, setup.e["desc"])
    assert (proof == setup.proof).all() and setup.verdict(proof) == 0


@pytest.mark.parametrize("case", tc.TAG_WORDS, ids=[r[0] for r in tc.TAG_WORDS])
def test_the_refusals_of_word_7(ctx, case):
    """on the host before anything is launched: the wire table and the output keep their words"""
    import sipp_amd
    _, desc, code = case
    s = lc.REFUSAL_SHAPE
    n = 1 << s["log_n"]
    gp = sipp_amd.PlonkParams(1, s["D"], s["C"])
    w = dev(np.full((s["num_wires"], n), 5, dtype=np.uint64))
    k = dev(np.zeros((s["num_constants"], n), dtype=np.uint64))
    out = dev(np.full((64, n), 9, dtype=np.uint64))
    words = (C.c_uint32 * 8)(*desc)
    ch = ctx._u64([3] * s["C"])
    rc_m = ctx.L.sipp_plonk_lookup_multiplicities(ctx.h, w.data_ptr(), k.data_ptr(), s["log_n"], s["num_wires"], s["num_constants"],
                                                  s["num_selectors"], words)
    rc_s = ctx.L.sipp_plonk_lookup_sums(ctx.h, w.data_ptr(), k.data_ptr(), s["log_n"], s["num_wires"], s["num_constants"],
                                        s["num_selectors"], C.byref(gp), words, ch, ch, out.data_ptr())
    assert (rc_m, rc_s) == ((code, code) if code is not None else (0, 0))
    if code is not None:
        assert (host(w) == 5).all() and (host(out) == 9).all()
    good_call(ctx)


class Setup:
    """the zero-constraint circuit (tests/_lookup_cases.py PROOF_*) over the tagged catalogue's largest entry"""

    def __init__(self, ctx):
        import sipp_amd
        from sipp_amd.circuit import fri_params
        self.e = e = tc.BY_NAME[tc.PROOF_ENTRY]()
        self.cs = lc.constants_sigmas(e)
        self.circ = sipp_amd.PlonkCircuit.from_dict(lc.proof_circuit(e))
        self.gp = sipp_amd.PlonkParams(lc.PROOF_ROUTED, e["D"], e["C"])
        self.fp = fri_params(e["log_n"], **lc.PROOF_FRI)
        self.wires = tc.multiplicities(e["desc"], e["wires"], e["consts"])
        _, self.cap, self._keep = ctx.commit_ex(dev(self.cs), e["log_n"], self.fp.rate_bits, self.fp.cap_height)
        self.proof = self.raw(ctx, self.wires, e["desc"])

    def raw(self, ctx, wires, desc):
        return ctx.plonk_prove_gates_lookup(dev(wires), dev(self.cs), self.e["log_n"], self.gp, self.fp, self.circ, lc.PROOF_DIGEST, [], desc)

    def verdict(self, proof, desc=None):
        import sipp_amd
        return sipp_amd.plonk_verify_gates_lookup(proof, self.cap, self.gp, self.fp, self.circ, lc.PROOF_DIGEST,
                                                  self.e["desc"] if desc is None else desc)


@pytest.fixture(scope="module")
def setup(ctx):
    return Setup(ctx)


def reading_verdict(proof, e):
    from sipp_amd.plonk_vanishing import _HostChallenger
    return tc.read_proof(proof, e, _HostChallenger())


def test_a_whole_tagged_proof_is_accepted_by_the_verifier_and_by_the_reading(setup):
    e = setup.e
    assert int(setup.proof[0]) == int.from_bytes(b"SIPPPLK4", "little") and [int(v) for v in setup.proof[16:24]] == list(e["desc"])
    assert setup.verdict(setup.proof) == 0
    assert reading_verdict(setup.proof, e) is None
    # under the same description without its tags: the header is not the caller's
    assert setup.verdict(setup.proof, e["desc"][:7] + (0,)) == 201
    bad = setup.proof.copy()
    bad[tc.tag_opening(e)] ^= np.uint64(1)                # the opened looking-tag column: every looking term depends on it
    assert setup.verdict(bad) == 210 and reading_verdict(bad, e) == "vanishing"


def test_circuit_data_proves_the_tagged_entry_on_all_three_paths(ctx, setup):
    import sipp_amd
    e = setup.e
    cd = sipp_amd.CircuitData(ctx, e["log_n"], setup.gp, setup.fp, setup.circ, setup.cs, [], digest=lc.PROOF_DIGEST)
    try:
        cd.set_lookup(e["desc"])
        cells = np.flatnonzero(e["wires"].reshape(-1)).astype(np.uint64)
        values = e["wires"].reshape(-1)[cells.astype(np.int64)]
        cd.set_input_map(cells, np.arange(len(cells), dtype=np.uint64), len(cells), 0)
        for proof in (cd.prove(e["wires"], []), cd.prove_inputs(cells, values, []), cd.prove_words(values, [], [])):
            assert len(proof) == len(setup.proof) and (proof == setup.proof).all()
            assert cd.verify(proof) == (0, 0)
        # a pair that only the other table holds: refused, and the same data proves the good entry afterwards
        bad = tc.pair_only_under_the_other_tag()
        w = e["wires"].copy()
        i = e["tables"][1][3][-1]
        x, y = e["entries"][0][-1]
        assert (x, y) not in e["entries"][1] and bad["expect"] == "absent"
        w[1][i], w[2][i] = x, y
        with pytest.raises(sipp_amd.SippError) as err:
            cd.prove(w, [])
        assert err.value.code == tc.E_WITNESS
        assert (cd.prove(e["wires"], []) == setup.proof).all()
    finally:
        cd.close()


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def gen_plans(e):
    """[(path, generators, schedule dict or None)]: row_local = sipp_plonk_generate_witness; coop / coop_rows = a schedule whose thin
    levels run plonk_witness_level_coop_kernel / _coop_rows_kernel (a swap generator no row holds chooses the latter); wide = the same
    through the 32-entry argument struct (seventeen generators, sixteen of them no row's)"""
    one = {"n_levels": 1, "rows": np.arange(1 << e["log_n"], dtype=np.uint32)[::-1].copy(),
           "level_offsets": np.array([0, 1 << e["log_n"]], dtype=np.uint32), "copy_src": np.zeros(0, dtype=np.uint64),
           "copy_dst": np.zeros(0, dtype=np.uint64), "copy_offsets": np.array([0, 0], dtype=np.uint32)}
    sc = e["sched"] if e["sched"] is not None else one
    gens = list(e["gens"])
    swap = (POSEIDON_SWAP, 0, tc.OTHER - 1, 0, 12, 29, 24, 25)
    fill = [(tc.GEN_LOOKUP, 0, tc.OTHER - 2 - q) + tc.GEN_SHAPE for q in range(16)]
    plans = [("coop", gens, sc), ("wide_args", fill[:8] + gens + fill[8:], sc)]
    if e["wires"].shape[0] >= 135:
        plans.append(("coop_rows", gens + [swap], sc))
    if e["sched"] is None or e["sched"]["n_levels"] == 1:
        plans.append(("row_local", gens, None))
    return plans


@pytest.mark.parametrize("name", [f.__name__ for f in tc.GEN_ENTRIES])
def test_the_generator_is_the_reading_cell_for_cell(ctx, name):
    """x = 0, T - 1, T, x and row0 given as value + p, an entry row at N, a T = 0 row (which comes back byte for byte), two tables of
    different row0 in one launch, a three-level chain, a level of 16384 rows: on every launch path, every cell of the table"""
    import sipp_amd
    e = tc.BY_NAME_GEN[name]()
    L = sipp_amd.lib()
    d_c = dev(e["consts"])
    try:
        for path, gens, sc in gen_plans(e):
            sched = sipp_amd.PlonkSchedule.from_dict(sc) if sc is not None else None
            for route in ((0,) if sched is None else (NO_GRAPH, 0, 0)):
                assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
                d_w = dev(e["wires"])
                if sched is None:
                    ctx.plonk_generate_witness(d_w, d_c, e["log_n"], gens, None)
                else:
                    ctx.plonk_generate_witness_levels(d_w, d_c, e["log_n"], gens, None, sched)
                ctx.sync()
                got = host(d_w)
                msg = tc.first_mismatch(got, e["expected"])
                assert msg is None, "%s route %d: %s" % (path, route, msg)
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_the_generator_beside_a_swap_generator_on_the_per_row_kernel(ctx):
    """gen_n8's rows in a table of 135 wires with a Poseidon swap generator in the list: thin levels then run
    plonk_witness_level_coop_rows_kernel, where the lookup rows are lane 0's"""
    import sipp_amd
    e = tc.gen_n8()
    w = np.zeros((135, 8), dtype=np.uint64)
    w[:6] = e["wires"]
    want = w.copy()
    want[:6] = e["expected"]
    gens = list(e["gens"]) + [(POSEIDON_SWAP, 0, tc.OTHER - 1, 0, 12, 29, 24, 25)]
    sc = {"n_levels": 1, "rows": np.arange(8, dtype=np.uint32), "level_offsets": np.array([0, 8], dtype=np.uint32),
          "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64), "copy_offsets": np.array([0, 0], dtype=np.uint32)}
    d_w = dev(w)
    ctx.plonk_generate_witness_levels(d_w, dev(e["consts"]), 3, gens, None, sipp_amd.PlonkSchedule.from_dict(sc))
    ctx.sync()
    msg = tc.first_mismatch(host(d_w), want)
    assert msg is None, msg


def test_the_generator_layout_refusals(ctx):
    """SIPP_E_BADARG before a launch on both entry points: the wire table keeps its words; the layout that ends where the table ends
    is served"""
    import sipp_amd
    e = tc.gen_n8()
    sc = sipp_amd.PlonkSchedule.from_dict({"n_levels": 1, "rows": np.arange(8, dtype=np.uint32), "level_offsets": np.array([0, 8], dtype=np.uint32),
                                           "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64),
                                           "copy_offsets": np.array([0, 0], dtype=np.uint32)})
    d_c = dev(e["consts"])
    for name, shape in tc.GEN_REFUSALS:
        for levels in (False, True):
            d_w = dev(e["wires"])
            with pytest.raises(sipp_amd.SippError) as err:
                if levels:
                    ctx.plonk_generate_witness_levels(d_w, d_c, 3, [(tc.GEN_LOOKUP, 0, 1) + shape], None, sc)
                else:
                    ctx.plonk_generate_witness(d_w, d_c, 3, [(tc.GEN_LOOKUP, 0, 1) + shape], None)
            assert err.value.code == tc.E_BADARG, name
            assert (host(d_w) == e["wires"]).all(), name
    for name, shape in tc.GEN_SERVED:
        gens = [(tc.GEN_LOOKUP, 0, 1) + shape]
        d_w = dev(e["wires"])
        ctx.plonk_generate_witness(d_w, d_c, 3, gens, None)
        ctx.sync()
        msg = tc.first_mismatch(host(d_w), tc.generate(e["wires"], e["consts"], gens)[0])
        assert msg is None, name + ": " + msg


# ---- the whole circuit ---------------------------------------------------------------------------------------------------------------------
def test_the_two_table_circuit_proves_on_all_three_paths(ctx):
    import sipp_amd
    from sipp_amd.circuit import CircuitProver, fri_params
    from tests._lookup_tables_circuit import XOR4, XorLookupCircuit
    circ = XorLookupCircuit()
    pr = CircuitProver(ctx, circ, fri=fri_params(circ.log_n, **lc.PROOF_FRI), params=sipp_amd.PlonkParams(circ.num_routed, 8, 2))
    try:
        assert pr.data.lookup == circ.lookup_description() and pr.data.lookup[7] != 0
        pr.data.set_input_map(*circ.words_map())
        a, b = 9, 12
        y = XOR4[16 * a + b]
        assert y == 5
        proof = pr.prove(y, a, b)
        assert int(proof[0]) == int.from_bytes(b"SIPPPLK4", "little") and int(proof[23]) == circ.lookup_description()[7]
        assert int(proof[-1]) == y and pr.verify(proof) == (0, 0)
        cells, values = circ.input_cells(y, a, b)
        for other in (pr.data.prove_inputs(cells, values, [y]), pr.data.prove_words(np.array([y, a, b], dtype=np.uint64), [], [y])):
            assert len(other) == len(proof) and (other == proof).all()
        # a = 16: outside the range table, and x = 16 a + b outside xor4 (the generator writes y = 0): refused; then a good proof again
        with pytest.raises(sipp_amd.SippError) as err:
            pr.prove(0, 16, b)
        assert err.value.code == tc.E_WITNESS
        again = pr.prove(XOR4[0x3c], 3, 12)
        assert pr.verify(again) == (0, 0) and int(again[-1]) == 15
        # a wrong public y: the word changed in a good proof, and a proof made for the wrong y (the copy constraint between the
        # generated y cell and the hashed public input does not hold)
        bad = proof.copy()
        bad[-1] ^= np.uint64(1)
        assert pr.verify(bad)[0] != 0
        try:
            wrong = pr.prove(y ^ 1, a, b)
        except sipp_amd.SippError:
            wrong = None
        assert wrong is None or pr.verify(wrong)[0] != 0
        assert (pr.prove(y, a, b) == proof).all()
    finally:
        pr.close()
