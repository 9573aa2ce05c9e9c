"""Zero-knowledge blinding on the device (sipp_amd/csrc/blind.hip and what rests on it) against the Python-integer reading of
tests/_blinding_cases.py: the salt columns and the SIPP_GEN_RANDOM rows word for word, the commitment over salt that sits in place,
whole "SIPPPLK5" proofs through the library's verifier and the composed reading, the circuit data's counter, the refusals."""
import numpy as np
import pytest

from tests import _blinding_cases as bc
from tests._device import NO_GRAPH, dev, first_mismatch, host

pytestmark = pytest.mark.gpu
POSEIDON_SWAP = 9                    # include/sipp_hip.h SIPP_GEN_POSEIDON_SWAP
SENTINEL = 0xDEADBEEF
OTHER = 0xFFFF                       # the selector value of rows no generator takes
D, NC = 8, 2                         # sipp_plonk_params of the whole proofs: max_degree, num_challenges


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=1 << 30)
    yield c
    c.close()


def blinding(counter=0, seed=bc.SEED):
    import sipp_amd
    return sipp_amd.Blinding.of(seed, counter)


# ---- salt -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter", bc.COUNTERS)
@pytest.mark.parametrize("ncols", [1, 137])
@pytest.mark.parametrize("log_m", [4, 7, 9, 10, 13])
def test_salt_columns_are_the_reading_word_for_word(ctx, log_m, ncols, counter):
    """fewer pairs than a wave, exactly one wave of pairs, the edges of a 256-lane block, many blocks; the polynomial columns in front
    keep their words"""
    m = 1 << log_m
    for stream in (1, 2, 3):
        buf = np.full((ncols + 4, m), SENTINEL, dtype=np.uint64)
        d = dev(buf)
        ctx.blind_salt(d, ncols, log_m, blinding(counter), stream)
        got = host(d)
        assert (got[:ncols] == SENTINEL).all(), "stream %d: a word in front of the salt changed" % stream
        assert first_mismatch(got[ncols:], bc.salt_columns(bc.SEED, counter, stream, m)) is None, stream


def test_a_sample_of_the_salt_is_block_in_python_integers(ctx):
    """the bulk reading goes through the C oracle's permutation: the device against block() itself at the first, an odd and the last leaf"""
    log_m, counter, stream = 10, bc.COUNTERS[1], 2
    d = dev(np.zeros((5, 1 << log_m), dtype=np.uint64))
    ctx.blind_salt(d, 1, log_m, blinding(counter), stream)
    got = host(d)[1:]
    for j in (0, 1, 513, (1 << log_m) - 1):
        want = bc.block(bc.SEED, counter, stream, j >> 1)[4 * (j & 1): 4 * (j & 1) + 4]
        assert [int(got[k][j]) for k in range(4)] == want, j


def test_a_commitment_over_salt_in_place_is_commit_ex_over_the_reading(ctx):
    """the wires oracle of a whole proof is committed from salt that sits in the LDE buffer in leaf order; its cap must be the cap
    sipp_commit_batch_ex gives for the reading's salt bit-reversed into natural order (see also the whole-proof tests)"""
    log_n, rate_bits, ncols = 10, 3, 9
    rng = np.random.default_rng(5)
    vals = rng.integers(0, bc.P, size=(ncols, 1 << log_n), dtype=np.uint64)
    salt = bc.salt_natural(bc.SEED, 3, bc.STREAM_WIRES, log_n + rate_bits)
    oracle, cap, keep = ctx.commit_ex(dev(vals), log_n, rate_bits, 4, salt=dev(salt))
    lde = host(keep[1])
    assert first_mismatch(lde[ncols:], bc.salt_columns(bc.SEED, 3, bc.STREAM_WIRES, 1 << (log_n + rate_bits))) is None
    # the same leaves hashed from a buffer whose salt the device drew: leaf order, no bit reversal
    d = dev(lde)
    d[ncols:] = 0
    ctx.blind_salt(d, ncols, log_n + rate_bits, blinding(3), bc.STREAM_WIRES)
    assert first_mismatch(host(d), lde) is None


# ---- SIPP_GEN_RANDOM ------------------------------------------------------------------------------------------------------------------------
def random_table(log_n, num_wires):
    n = 1 << log_n
    consts = np.full((1, n), OTHER, dtype=np.uint64)
    consts[0][sorted({r for r in (0, 1, 63, 64, 255, 256, n - 1) if r < n})] = 3
    return np.full((num_wires, n), SENTINEL, dtype=np.uint64), consts


@pytest.mark.parametrize("shape", [(0, 1), (3, 8), (7, 9), (2, 136)], ids=["1_wire", "8_wires_across_two_blocks", "9_wires", "136_wires"])
def test_random_rows_are_the_reading_on_every_path(ctx, shape):
    """rows 0 and N - 1 among them; both entry points; the level kernels' narrow and wide argument structs and the per-row kernel, through
    the captured graph, its replay and launch by launch; every other cell keeps its word"""
    import sipp_amd
    log_n = 9
    w, consts = random_table(log_n, 140)
    gen = (bc.GEN_RANDOM, 0, 3) + shape + (0, 0, 0)
    fill = [(bc.GEN_RANDOM, 0, OTHER - 2 - q, 0, 140, 0, 0, 0) for q in range(16)]
    swap = (POSEIDON_SWAP, 0, OTHER - 1, 0, 12, 29, 24, 25)
    one = {"n_levels": 1, "rows": np.arange(1 << log_n, dtype=np.uint32)[::-1].copy(), "level_offsets": np.array([0, 1 << log_n], dtype=np.uint32),
           "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64), "copy_offsets": np.array([0, 0], dtype=np.uint32)}
    L = sipp_amd.lib()
    d_c = dev(consts)
    try:
        for counter in bc.COUNTERS:
            want, mask = bc.blind_fill(w, consts, [gen], bc.SEED, counter)
            assert mask.sum() == int((consts[0] == 3).sum()) * shape[1] and (want[~mask] == SENTINEL).all()
            for path, gens, sc in (("coop", [gen], one), ("wide_args", fill[:8] + [gen] + fill[8:], one), ("coop_rows", [gen, swap], one),
                                   ("row_local", [gen], None)):
                sched = sipp_amd.PlonkSchedule.from_dict(sc) if sc is not None else None
                for route in ((0,) if sched is None else (NO_GRAPH, 0, 0)):
                    assert L.sipp_ctx_set_kernel_routes(ctx.h, route) == 0
                    d_w = dev(w)
                    if sched is None:
                        ctx.plonk_generate_witness(d_w, d_c, log_n, gens, None, blind=blinding(counter))
                    else:
                        ctx.plonk_generate_witness_levels(d_w, d_c, log_n, gens, None, sched, blind=blinding(counter))
                    ctx.sync()
                    msg = first_mismatch(host(d_w), want)
                    assert msg is None, "%s route %d counter %d: %s" % (path, route, counter, msg)
    finally:
        assert L.sipp_ctx_set_kernel_routes(ctx.h, 0) == 0


def test_a_random_generator_without_a_seed_or_outside_the_table_is_refused(ctx):
    import sipp_amd
    w, consts = random_table(4, 12)
    sc = sipp_amd.PlonkSchedule.from_dict({"n_levels": 1, "rows": np.arange(16, dtype=np.uint32), "level_offsets": np.array([0, 16], dtype=np.uint32),
                                           "copy_src": np.zeros(0, dtype=np.uint64), "copy_dst": np.zeros(0, dtype=np.uint64),
                                           "copy_offsets": np.array([0, 0], dtype=np.uint32)})
    d_c = dev(consts)
    good = (bc.GEN_RANDOM, 0, 3, 4, 8, 0, 0, 0)                     # ends where the table ends: served
    cases = [("no_seed", good, None), ("one_wire_past_the_table", (bc.GEN_RANDOM, 0, 3, 5, 8, 0, 0, 0), blinding()),
             ("first_wire_huge", (bc.GEN_RANDOM, 0, 3, 0xFFFFFFFF, 2, 0, 0, 0), blinding()),
             ("seed_word_p", good, blinding(0, (bc.P, 0, 0, 0)))]
    for name, gen, bl in cases:
        for levels in (False, True):
            d_w = dev(w)
            with pytest.raises(sipp_amd.SippError) as err:
                if levels:
                    ctx.plonk_generate_witness_levels(d_w, d_c, 4, [gen], None, sc, blind=bl)
                else:
                    ctx.plonk_generate_witness(d_w, d_c, 4, [gen], None, blind=bl)
            assert err.value.code == bc.E_BADARG, name
            assert (host(d_w) == w).all(), name
    d_w = dev(w)
    ctx.plonk_generate_witness(d_w, d_c, 4, [good], None, blind=blinding())
    ctx.sync()
    assert first_mismatch(host(d_w), bc.blind_fill(w, consts, [good], bc.SEED, 0)[0]) is None


# ---- whole proofs -----------------------------------------------------------------------------------------------------------------------------
class Setup:
    """the catalogue's circuit at log_n = 10 through the raw calls: the witness generated on the device under (SEED, counter), the
    multiplicities with lookups, sipp_plonk_prove_gates_zk"""

    def __init__(self, ctx, lookups):
        import sipp_amd
        self.c = c = bc.circuit(lookups)
        self.circ = c.circuit()
        self.desc = tuple(self.circ.get("lookup", (0,) * 8))
        self.pc = sipp_amd.PlonkCircuit.from_dict(self.circ)
        self.gp = sipp_amd.PlonkParams(c.num_routed, D, NC)
        self.fp, self.fp_plain = bc.proof_fri(c.log_n, 1), bc.proof_fri(c.log_n, 0)
        self.cs = c.constants_sigmas()
        self.d_cs = dev(self.cs)
        _, self.cap, self._keep = ctx.commit_ex(self.d_cs, c.log_n, self.fp.rate_bits, self.fp.cap_height)
        self.sched = sipp_amd.PlonkSchedule.from_dict(c.schedule())
        self.a, self.b = 9, 12
        self.y = c.value(self.a, self.b)
        self.pis = c.public_inputs(self.y)

    def witness(self, ctx, counter):
        from tests import _oracle as orc
        d_w = dev(self.c.partial_witness(self.y, self.a, self.b))
        pih = [int(x) for x in orc.hash_no_pad(self.pis)]
        ctx.plonk_generate_witness_levels(d_w, self.d_cs[:self.circ["num_constants"]], self.c.log_n, self.c.generators(), pih, self.sched,
                                          blind=blinding(counter))
        if any(self.desc):
            ctx.plonk_lookup_multiplicities(d_w, self.d_cs[:self.circ["num_constants"]], self.c.log_n, self.circ["num_selectors"], self.desc)
        return d_w

    def prove(self, ctx, counter, d_w=None):
        d_w = self.witness(ctx, counter) if d_w is None else d_w
        return ctx.plonk_prove_gates_zk(d_w, self.d_cs, self.c.log_n, self.gp, self.fp, self.pc, bc.PROOF_DIGEST, self.pis, self.desc,
                                        blinding(counter))

    def verdict(self, proof, fp=None):
        import sipp_amd
        return sipp_amd.plonk_verify_gates_lookup(proof, self.cap, self.gp, self.fp if fp is None else fp, self.pc, bc.PROOF_DIGEST, self.desc)

    def reading(self, proof):
        return bc.read_proof5(proof, self.circ, self.cap, bc.PROOF_DIGEST, self.fp, D, NC, len(self.pis))


@pytest.fixture(scope="module", params=[False, True], ids=["no_lookups", "lookups"])
def setup(ctx, request):
    s = Setup(ctx, request.param)
    s.proof = s.prove(ctx, 0)
    return s


def test_a_whole_proof_is_accepted_by_the_verifier_and_by_the_reading(setup):
    p = setup.proof
    assert int(p[0]) == bc.MAGIC5 and int(p[12]) == 1 and [int(v) for v in p[16:24]] == list(setup.desc)
    assert int(p[-1]) == setup.y
    assert setup.verdict(p) == 0
    assert setup.reading(p) is None
    assert setup.verdict(p, setup.fp_plain) == 201


def test_the_wires_cap_is_commit_ex_over_the_readings_rows_and_salt(ctx, setup):
    c = setup.c
    table = host(setup.witness(ctx, 0))
    want, mask = bc.blind_fill(table, setup.cs[:setup.circ["num_constants"]], c.generators(), bc.SEED, 0)
    # the second row of every pair holds copies in its routed wires: those cells are not the generator's any more
    for _, b in c.blind_rows["pairs"]:
        mask[:c.num_routed, b] = False
    assert mask.sum() > 0 and (table[mask] == want[mask]).all()
    for a, b in c.blind_rows["pairs"]:
        assert (table[:c.num_routed, a] == table[:c.num_routed, b]).all()
    table[mask] = want[mask]
    salt = bc.salt_natural(bc.SEED, 0, bc.STREAM_WIRES, c.log_n + setup.fp.rate_bits)
    _, cap, _keep = ctx.commit_ex(dev(table), c.log_n, setup.fp.rate_bits, setup.fp.cap_height, salt=dev(salt))
    n_cap = 4 << setup.fp.cap_height
    assert (setup.proof[24:24 + n_cap] == cap.reshape(-1)).all()


def test_every_query_round_opens_the_readings_salt(setup):
    rounds = bc.query_rounds(setup.proof, setup.circ, bc.PROOF_DIGEST, setup.fp, D, NC, len(setup.pis))
    assert len(rounds) == setup.fp.num_queries
    m = 1 << (setup.c.log_n + setup.fp.rate_bits)
    for x, leaves, _ in rounds:
        for o, stream in ((1, bc.STREAM_WIRES), (2, bc.STREAM_ZS), (3, bc.STREAM_QUOTIENT)):
            want = bc.block(bc.SEED, 0, stream, x >> 1)[4 * (x & 1): 4 * (x & 1) + 4]
            assert leaves[o][-4:] == want, (x, o)
            assert leaves[o][-4:] == [int(v) for v in bc.salt_columns(bc.SEED, 0, stream, m)[:, x]]


def test_seed_and_counter_fix_the_proof_and_the_next_counter_changes_it(ctx, setup):
    assert (setup.prove(ctx, 0) == setup.proof).all()
    other = setup.prove(ctx, 1)
    assert setup.verdict(other) == 0 and len(other) == len(setup.proof)
    n_cap = 4 << setup.fp.cap_height
    for o in range(3):
        assert (other[24 + o * n_cap: 24 + (o + 1) * n_cap] != setup.proof[24 + o * n_cap: 24 + (o + 1) * n_cap]).any(), o
    s0 = bc.parse5(setup.proof, setup.circ, setup.fp, D, NC, 1)
    s1 = bc.parse5(other, setup.circ, setup.fp, D, NC, 1)
    K, R, W = setup.circ["num_constants"], setup.c.num_routed, setup.circ["num_wires"]
    for k in list(range(K + R, K + R + W)) + list(range(K + R + W, K + R + W + NC)):        # every wire column, every Z column, at zeta
        assert s0["opened"][k] != s1["opened"][k], k
    assert s0["pis"] == s1["pis"]


def test_without_a_seed_the_call_is_the_lookup_prover_byte_for_byte(ctx, setup):
    d_w = setup.witness(ctx, 0)
    plain = ctx.plonk_prove_gates_lookup(d_w, setup.d_cs, setup.c.log_n, setup.gp, setup.fp_plain, setup.pc, bc.PROOF_DIGEST, setup.pis, setup.desc)
    same = ctx.plonk_prove_gates_zk(d_w, setup.d_cs, setup.c.log_n, setup.gp, setup.fp_plain, setup.pc, bc.PROOF_DIGEST, setup.pis, setup.desc, None)
    assert len(plain) == len(same) and (plain == same).all()
    assert int(plain[0]) == int.from_bytes(b"SIPPPLK4" if any(setup.desc) else b"SIPPPLK3", "little")
    assert setup.verdict(plain, setup.fp_plain) == 0 and setup.verdict(plain) == 201


# ---- circuit data ---------------------------------------------------------------------------------------------------------------------------
def test_circuit_data_counts_its_proofs(ctx, setup):
    import sipp_amd
    from sipp_amd.circuit import CircuitProver
    c = setup.c
    pr = CircuitProver(ctx, c, fri=bc.proof_fri(c.log_n, 0), params=setup.gp, digest=bc.PROOF_DIGEST, zero_knowledge=True, seed=bc.SEED)
    try:
        assert pr.fri.hiding == 1
        first = pr.prove(setup.y, setup.a, setup.b)                                   # counter 0
        assert len(first) == len(setup.proof) and (first == setup.proof).all()
        second = pr.prove(setup.y, setup.a, setup.b)                                  # counter 1
        assert (second != first).any() and pr.verify(first) == (0, 0) and pr.verify(second) == (0, 0)
        assert (second == setup.prove(ctx, 1)).all()
        cells, values = c.input_cells(setup.y, setup.a, setup.b)
        pr.data.set_input_map(*c.words_map())
        for path in ("dense", "inputs", "words"):
            pr.data.set_blinding(bc.SEED)                                             # back to counter 0
            proof = {"dense": lambda: pr.prove(setup.y, setup.a, setup.b), "inputs": lambda: pr.data.prove_inputs(cells, values, setup.pis),
                     "words": lambda: pr.data.prove_words(np.array([setup.y, setup.a, setup.b], dtype=np.uint64), [], setup.pis)}[path]()
            assert len(proof) == len(first) and (proof == first).all(), path
        # a refusal uses its number up: the next proof is counter 2's
        pr.data.set_blinding(bc.SEED)
        pr.prove(setup.y, setup.a, setup.b)
        with pytest.raises(sipp_amd.SippError) as err:
            pr.data.prove_inputs(np.array([1 << 62], dtype=np.uint64), np.array([0], dtype=np.uint64), setup.pis)
        assert err.value.code == bc.E_BADARG
        assert (pr.prove(setup.y, setup.a, setup.b) == setup.prove(ctx, 2)).all()
    finally:
        pr.close()


def test_circuit_data_refusals(ctx, setup):
    import sipp_amd
    c = setup.c
    hiding = sipp_amd.CircuitData(ctx, c.log_n, setup.gp, setup.fp, setup.pc, setup.cs, c.generators(), sched=c.schedule(), digest=bc.PROOF_DIGEST)
    plain = sipp_amd.CircuitData(ctx, c.log_n, setup.gp, setup.fp_plain, setup.pc, setup.cs, c.generators(), sched=c.schedule(),
                                 digest=bc.PROOF_DIGEST)
    try:
        if any(setup.desc):
            hiding.set_lookup(setup.desc)
        w = c.partial_witness(setup.y, setup.a, setup.b)
        with pytest.raises(sipp_amd.SippError) as err:                    # hiding, no seed
            hiding.prove(w, setup.pis)
        assert err.value.code == bc.E_BADARG
        with pytest.raises(sipp_amd.SippError) as err:                    # a seed on a data that is not hiding
            plain.set_blinding(bc.SEED)
        assert err.value.code == bc.E_BADARG
        with pytest.raises(sipp_amd.SippError) as err:                    # a seed word that is no field element
            hiding.set_blinding((0, 0, bc.P, 0))
        assert err.value.code == bc.E_BADARG
        hiding.set_blinding(bc.SEED)
        proof = hiding.prove(w, setup.pis)
        assert (proof == setup.proof).all() and hiding.verify(proof) == (0, 0)
        assert plain.verify(proof) == (bc.E_VERIFY, 201)
    finally:
        hiding.close()
        plain.close()


# ---- the refusals of the prover -----------------------------------------------------------------------------------------------------------
def test_the_prover_refuses_seed_and_hiding_that_disagree(ctx, setup):
    import sipp_amd
    d_w = setup.witness(ctx, 0)
    args = (d_w, setup.d_cs, setup.c.log_n, setup.gp)
    tail = (setup.pc, bc.PROOF_DIGEST, setup.pis, setup.desc)
    with pytest.raises(sipp_amd.SippError) as err:                        # a seed, hiding = 0
        ctx.plonk_prove_gates_zk(*args, setup.fp_plain, *tail, blinding())
    assert err.value.code == bc.E_BADARG
    with pytest.raises(sipp_amd.SippError) as err:                        # hiding = 1, no seed
        ctx.plonk_prove_gates_zk(*args, setup.fp, *tail, None)
    assert err.value.code == bc.E_BADARG
    with pytest.raises(sipp_amd.SippError) as err:                        # the older entry keeps its answer to a hiding fp
        ctx.plonk_prove_gates_lookup(*args, setup.fp, *tail)
    assert err.value.code == bc.E_UNSUPPORTED
    with pytest.raises(sipp_amd.SippError) as err:                        # a seed word >= p
        ctx.plonk_prove_gates_zk(*args, setup.fp, *tail, blinding(0, (1, 2, 3, bc.P)))
    assert err.value.code == bc.E_BADARG
    # a pre-committed wires oracle: unsalted under blinding, salted without
    table = host(d_w)
    salt = bc.salt_natural(bc.SEED, 0, bc.STREAM_WIRES, setup.c.log_n + setup.fp.rate_bits)
    bare, bare_cap, _k0 = ctx.commit_ex(dev(table), setup.c.log_n, setup.fp.rate_bits, setup.fp.cap_height)
    salted, salted_cap, _k1 = ctx.commit_ex(dev(table), setup.c.log_n, setup.fp.rate_bits, setup.fp.cap_height, salt=dev(salt))
    with pytest.raises(sipp_amd.SippError) as err:
        ctx.plonk_prove_gates_zk(*args, setup.fp, *tail, blinding(), wires_oracle=bare, wires_cap=bare_cap)
    assert err.value.code == bc.E_BADARG
    with pytest.raises(sipp_amd.SippError) as err:
        ctx.plonk_prove_gates_zk(*args, setup.fp_plain, *tail, None, wires_oracle=salted, wires_cap=salted_cap)
    assert err.value.code == bc.E_BADARG
    # the ctx is usable: the salted oracle the caller committed gives the proof the prover's own commitment gives
    again = ctx.plonk_prove_gates_zk(*args, setup.fp, *tail, blinding(), wires_oracle=salted, wires_cap=salted_cap)
    assert (again == setup.proof).all()
    assert (setup.prove(ctx, 0) == setup.proof).all()
