"""The lookup argument on the device (sipp_amd/csrc/lookup.hip) on the catalogue of tests/_lookup_cases.py: the multiplicities and
the running-sum columns S / U word for word against the catalogue's Python-integer reading, for every entry; the two witness refusals
(a pair in no table slot, theta on a combination) and the description refusals by their exact codes, each followed by a good call on
the same ctx.  Whole proofs (log_n = 10, rate_bits 3, cap height 4, 8 queries): the raw call and CircuitData on its three prove paths,
accepted by the library's verifier and by the reading's vanishing equation from the opened values; spoiled multiplicities; an empty
description against sipp_plonk_prove_gates word for word; a CircuitBuilder range-check circuit."""
import ctypes as C

import numpy as np
import pytest

from tests import _lookup_cases as lc
from tests._device import dev, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def device_multiplicities(ctx, e):
    return host(ctx.plonk_lookup_multiplicities(dev(e["wires"]), dev(e["consts"]), e["log_n"], e["num_selectors"], e["desc"]))


def device_sums(ctx, e, wires):
    import sipp_amd
    gp = sipp_amd.PlonkParams(1, e["D"], e["C"])
    return host(ctx.plonk_lookup_sums(dev(wires), dev(e["consts"]), e["log_n"], e["num_selectors"], gp, e["desc"], e["etas"], e["thetas"]))


def good_call(ctx):
    e = lc.BY_NAME[lc.GOOD_AFTER_REFUSAL]()
    want = lc.multiplicities(e["desc"], e["wires"], e["consts"])
    msg = lc.first_mismatch(device_multiplicities(ctx, e), want)
    assert msg is None, "after the refusal: " + msg
    cols, _ = lc.sums(e["desc"], want, e["consts"], e["D"], e["etas"], e["thetas"])
    msg = lc.first_mismatch(device_sums(ctx, e, want), cols)
    assert msg is None, "after the refusal: " + msg


@pytest.mark.parametrize("name", lc.IDS)
def test_multiplicities_and_sums_are_the_readings(ctx, name):
    """the entry's tables as they are (garbage in the m cells and in unmarked rows, non-canonical words included): every wire cell
    after the multiplicities, then every S / U cell from the device's own multiplicities"""
    e = lc.BY_NAME[name]()
    want = lc.multiplicities(e["desc"], e["wires"], e["consts"])
    got = device_multiplicities(ctx, e)
    msg = lc.first_mismatch(got, want)
    assert msg is None, msg
    cols, closes = lc.sums(e["desc"], want, e["consts"], e["D"], e["etas"], e["thetas"])
    assert closes
    msg = lc.first_mismatch(device_sums(ctx, e, got), cols)
    assert msg is None, msg


def good_proof(ctx, setup):
    """the same ctx proves a good case: the raw proof again, word for word, accepted"""
    proof = setup.raw(ctx, setup.wires, setup.e["desc"])
    assert (proof == setup.proof).all() and setup.verdict(proof) == 0


def test_a_pair_in_no_table_slot_is_refused(ctx, setup):
    import sipp_amd
    e = lc.absent_pair()
    with pytest.raises(sipp_amd.SippError) as err:
        device_multiplicities(ctx, e)
    assert err.value.code == lc.E_WITNESS
    good_call(ctx)
    good_proof(ctx, setup)


@pytest.mark.parametrize("name", ["theta_on_a_looking_combination", "theta_on_a_table_combination"])
def test_theta_on_a_combination_is_refused(ctx, setup, name):
    import sipp_amd
    e = lc.BY_NAME[name]()
    wires = lc.multiplicities(e["desc"], e["wires"], e["consts"])
    msg = lc.first_mismatch(device_multiplicities(ctx, e), wires)
    assert msg is None, msg
    with pytest.raises(sipp_amd.SippError) as err:
        device_sums(ctx, e, wires)
    assert err.value.code == lc.E_WITNESS
    good_call(ctx)
    good_proof(ctx, setup)


@pytest.mark.parametrize("case", lc.REFUSALS, ids=[r[0] for r in lc.REFUSALS])
def test_description_refusals(ctx, case):
    """refused on the host before anything is launched: the wire table and the output keep their words; the ctx computes afterwards"""
    import sipp_amd
    _, desc, code = case
    s = lc.REFUSAL_SHAPE
    n = 1 << s["log_n"]
    gp = sipp_amd.PlonkParams(1, s["D"], s["C"])
    w = dev(np.full((s["num_wires"], n), 5, dtype=np.uint64))
    k = dev(np.zeros((s["num_constants"], n), dtype=np.uint64))
    out = dev(np.full((64, n), 9, dtype=np.uint64))
    words = (C.c_uint32 * 8)(*desc)
    assert ctx.L.sipp_plonk_lookup_multiplicities(ctx.h, w.data_ptr(), k.data_ptr(), s["log_n"], s["num_wires"], s["num_constants"],
                                                  s["num_selectors"], words) == code
    ch = ctx._u64([3] * s["C"])
    assert ctx.L.sipp_plonk_lookup_sums(ctx.h, w.data_ptr(), k.data_ptr(), s["log_n"], s["num_wires"], s["num_constants"],
                                        s["num_selectors"], C.byref(gp), words, ch, ch, out.data_ptr()) == code
    assert (host(w) == 5).all() and (host(out) == 9).all()
    # the same shape with a description that fits is served (no table row, no looking row: nothing to count, every column 0)
    good = (C.c_uint32 * 8)(*lc.GOOD_DESC)
    assert ctx.L.sipp_plonk_lookup_multiplicities(ctx.h, w.data_ptr(), k.data_ptr(), s["log_n"], s["num_wires"], s["num_constants"],
                                                  s["num_selectors"], good) == 0
    good_call(ctx)


def test_a_marker_that_is_neither_0_nor_1_is_refused(ctx):
    e = dict(lc.BY_NAME[lc.GOOD_AFTER_REFUSAL]())
    consts = e["consts"].copy()
    consts[e["desc"][3]][e["table_rows"][0]] = 2
    e["consts"] = consts
    import sipp_amd
    with pytest.raises(sipp_amd.SippError) as err:
        device_multiplicities(ctx, e)
    assert err.value.code == lc.E_BADARG
    good_call(ctx)


def test_an_empty_description_does_nothing(ctx):
    e = lc.BY_NAME[lc.GOOD_AFTER_REFUSAL]()
    desc = (0,) * 8
    got = host(ctx.plonk_lookup_multiplicities(dev(e["wires"]), dev(e["consts"]), e["log_n"], e["num_selectors"], desc))
    assert (got == e["wires"]).all()


# ---- whole proofs: log_n = 10, rate_bits 3, cap height 4, 8 queries ----------------------------------------------------------------------
class Setup:
    """the zero-constraint circuit over the catalogue's largest entry (tests/_lookup_cases.py PROOF_*), shared by the tests below and
    never written: the tables on the host, the circuit, the parameters, the constants_sigmas cap"""

    def __init__(self, ctx):
        import sipp_amd
        from sipp_amd.circuit import fri_params
        self.e = e = lc.BY_NAME[lc.PROOF_ENTRY]()
        self.cs = lc.constants_sigmas(e)
        self.circ = sipp_amd.PlonkCircuit.from_dict(lc.proof_circuit(e))
        self.gp = sipp_amd.PlonkParams(lc.PROOF_ROUTED, e["D"], e["C"])
        self.fp = fri_params(e["log_n"], **lc.PROOF_FRI)
        self.wires = lc.multiplicities(e["desc"], e["wires"], e["consts"])
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
    return lc.read_proof(proof, e, _HostChallenger())


def test_the_raw_proof_is_accepted_by_the_verifier_and_by_the_reading(setup):
    assert int(setup.proof[0]) == int.from_bytes(b"SIPPPLK4", "little") and int(setup.proof[5]) == len(setup.proof)
    assert [int(v) for v in setup.proof[16:24]] == list(setup.e["desc"])
    assert setup.verdict(setup.proof) == 0
    assert reading_verdict(setup.proof, setup.e) is None


def test_a_flipped_s_opening_is_refused_by_both(setup):
    e = setup.e
    K, W = e["consts"].shape[0], e["wires"].shape[0]
    at = 24 + 12 * (1 << lc.PROOF_FRI["cap_height"]) + 8 + 2 * (K + lc.PROOF_ROUTED + W + e["C"] * 1)      # S_0(zeta), behind Z_0, Z_1
    bad = setup.proof.copy()
    bad[at] ^= np.uint64(1)
    assert setup.verdict(bad) == 210
    assert reading_verdict(bad, e) == "vanishing"


def test_spoiled_multiplicities_do_not_end_in_an_accepted_proof(ctx, setup):
    """one multiplicity moved from an entry to another: the sum no longer closes, the quotient is no polynomial of its degree"""
    import sipp_amd
    e = setup.e
    tm = e["desc"][5]
    wires = setup.wires.copy()
    i = e["table_rows"][0]
    wires[tm][i] = (int(wires[tm][i]) + 1) % lc.P
    try:
        proof = setup.raw(ctx, wires, e["desc"])
    except sipp_amd.SippError:
        return
    assert setup.verdict(proof) != 0
    assert reading_verdict(proof, e) is not None


def test_an_empty_description_gives_prove_gates_proof_word_for_word(ctx, setup):
    e = setup.e
    want = ctx.plonk_prove_gates(dev(setup.wires), dev(setup.cs), e["log_n"], setup.gp, setup.fp, setup.circ, lc.PROOF_DIGEST, [])
    got = setup.raw(ctx, setup.wires, (0,) * 8)
    assert int(got[0]) == int.from_bytes(b"SIPPPLK3", "little")
    assert len(got) == len(want) and (got == want).all()
    assert setup.verdict(got, (0,) * 8) == 0 and setup.verdict(got) != 0 and setup.verdict(setup.proof, (0,) * 8) != 0


def test_circuit_data_proves_on_all_three_paths(ctx, setup):
    """CircuitData with the description set: the multiplicities run behind (here empty) witness generation on the device, from the
    entry's wire table with GARBAGE in the m cells; each path's proof is the raw call's word for word, and verify() accepts it"""
    import sipp_amd
    e = setup.e
    cd = sipp_amd.CircuitData(ctx, e["log_n"], setup.gp, setup.fp, setup.circ, setup.cs, [], digest=lc.PROOF_DIGEST)
    try:
        assert (cd.cap == setup.cap).all()
        cd.set_lookup(e["desc"])
        cells = np.flatnonzero(e["wires"].reshape(-1)).astype(np.uint64)
        values = e["wires"].reshape(-1)[cells.astype(np.int64)]
        cd.set_input_map(cells, np.arange(len(cells), dtype=np.uint64), len(cells), 0)
        for proof in (cd.prove(e["wires"], []), cd.prove_inputs(cells, values, []), cd.prove_words(values, [], [])):
            assert len(proof) == len(setup.proof) and (proof == setup.proof).all()
            assert cd.verify(proof) == (0, 0)
        # a pair outside the table: refused, no proof; the same data proves afterwards
        w = e["wires"].copy()
        lw, n_look = e["desc"][1], e["desc"][2]
        w[lw + 2 * (n_look - 1)][e["look_rows"][-1]] = 0x12345
        with pytest.raises(sipp_amd.SippError) as err:
            cd.prove(w, [])
        assert err.value.code == lc.E_WITNESS
        assert (cd.prove(e["wires"], []) == setup.proof).all()
        # taken off again: the circuit proves without the argument
        cd.set_lookup((0,) * 8)
        assert int(cd.prove(setup.wires, [])[0]) == int.from_bytes(b"SIPPPLK3", "little")
    finally:
        cd.close()


# ---- builder level ---------------------------------------------------------------------------------------------------------------------
def test_a_range_check_circuit_proves_and_a_value_outside_the_table_is_refused(ctx):
    import sipp_amd
    from sipp_amd.circuit import CircuitProver, fri_params
    from tests._lookup_circuit import RangeCheckCircuit
    circ = RangeCheckCircuit(n_values=11, bits=5)
    pr = CircuitProver(ctx, circ, fri=fri_params(circ.log_n, **lc.PROOF_FRI), params=sipp_amd.PlonkParams(circ.num_routed, 8, 2))
    try:
        assert pr.data.lookup == circ.lookup_description() and any(pr.data.lookup)
        proof = pr.prove([3, 31, 0, 7, 7, 7, 30, 1, 2, 16, 15])
        assert int(proof[0]) == int.from_bytes(b"SIPPPLK4", "little")
        assert pr.verify(proof) == (0, 0)
        bad = proof.copy()
        bad[len(bad) // 2] ^= np.uint64(1)
        assert pr.verify(bad)[0] != 0
        with pytest.raises(sipp_amd.SippError) as err:
            pr.prove([3, 31, 0, 7, 7, 7, 30, 1, 2, 16, 32])
        assert err.value.code == lc.E_WITNESS
        assert pr.verify(pr.prove([0] * 11)) == (0, 0)
    finally:
        pr.close()
