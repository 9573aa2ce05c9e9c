"""The sibling entries of the outer prover held together in one table (sipp_amd/csrc/plonk.hip, circuit_data.hip): every
sipp_plonk_prove_gates* entry with its option off is the entry beside it, word for word, and the oracle's proof; a circuit data proves what
the matching direct entry proves from the same wire table, seed and counter, and sizes its buffer as that entry's size function does; a
hiding fp without a seed, and a seed with a plain fp, get from each entry the code that entry has always answered.  The circuit is the
blinding catalogue's (tests/_blinding_cases.py, log_n = 10).  Every refusal here is a host-side argument check: nothing is launched."""
import ctypes as C

import pytest

from tests import _blinding_cases as bc
from tests import _oracle
from tests._device import dev, host

pytestmark = pytest.mark.gpu
D, NC = 8, 2                         # sipp_plonk_params: max_degree, num_challenges
A, B = 9, 12                         # the witness inputs
NONE = (0,) * 8                      # the empty lookup description


@pytest.fixture(scope="module")
def ctx():
    import sipp_amd
    c = sipp_amd.Ctx(workspace_bytes=2 << 30)
    yield c
    c.close()


def blinding(counter=0):
    import sipp_amd
    return sipp_amd.Blinding.of(bc.SEED, counter)


class Case:
    """one kind of proof: the circuit with its wire table generated on the device (the multiplicities filled in with lookups)"""

    def __init__(self, ctx, lookups, blinded):
        import sipp_amd
        self.c = c = bc.circuit(lookups, blind=blinded)
        self.circ = c.circuit()
        self.desc = tuple(self.circ["lookup"]) if lookups else NONE
        self.pc = sipp_amd.PlonkCircuit.from_dict(self.circ)
        self.gp = sipp_amd.PlonkParams(c.num_routed, D, NC)
        self.fp, self.fp_plain, self.fp_hiding = bc.proof_fri(c.log_n, 1 if blinded else 0), bc.proof_fri(c.log_n, 0), bc.proof_fri(c.log_n, 1)
        self.blind = blinding() if blinded else None
        self.cs = c.constants_sigmas()
        self.d_cs = dev(self.cs)
        self.y = c.value(A, B)
        self.pis = c.public_inputs(self.y)
        K = self.circ["num_constants"]
        self.d_w = dev(c.partial_witness(self.y, A, B))
        pih = [int(x) for x in _oracle.hash_no_pad(self.pis)]
        ctx.plonk_generate_witness_levels(self.d_w, self.d_cs[:K], c.log_n, c.generators(), pih, sipp_amd.PlonkSchedule.from_dict(c.schedule()),
                                          blind=self.blind)
        if lookups:
            ctx.plonk_lookup_multiplicities(self.d_w, self.d_cs[:K], c.log_n, self.circ["num_selectors"], self.desc)

    def head(self, fp=None):
        """the arguments every direct entry starts with"""
        return (self.d_w, self.d_cs, self.c.log_n, self.gp, self.fp if fp is None else fp, self.pc, bc.PROOF_DIGEST, self.pis)

    def size(self, L, which, fp=None):
        """sipp_plonk_gates{,_lookup,_zk}_proof_size for this circuit and description"""
        args = [self.c.log_n, C.byref(self.gp), C.byref(self.fp if fp is None else fp), C.byref(self.pc), len(self.pis)]
        if which != "gates":
            args.append((C.c_uint32 * 8)(*self.desc))
        return int(getattr(L, "sipp_plonk_%s_proof_size" % which)(*args))


def same(got, want):
    return len(got) == len(want) and bool((got == want).all())


def test_with_every_option_off_the_four_entries_give_the_oracles_proof(ctx):
    k = Case(ctx, False, False)
    proofs = {"gates": ctx.plonk_prove_gates(*k.head()), "lookup": ctx.plonk_prove_gates_lookup(*k.head(), NONE),
              "zk": ctx.plonk_prove_gates_zk(*k.head(), NONE, None), "h": ctx.plonk_prove_gates_h(*k.head(), None, None, "poseidon")}
    want = _oracle.plonk_prove_gates(host(k.d_w), k.cs, k.c.log_n, _oracle.plonk_params(k.c.num_routed, D, NC), bc.orc_fri(k.fp), k.circ,
                                     bc.PROOF_DIGEST, k.pis)
    for name, got in proofs.items():
        assert same(got, proofs["gates"]), name
        assert same(got, want), name
    sizes = [k.size(ctx.L, which) for which in ("gates", "gates_lookup", "gates_zk")]
    assert sizes[0] == sizes[1] == sizes[2] and sizes[0] >= len(want) > 0


# kind -> (lookups, blinded, the circuit data's hasher (None: sipp_circuit_build), the direct entry, its size function)
KINDS = {
    "plain": (False, False, None, lambda ctx, k: ctx.plonk_prove_gates(*k.head()), "gates"),
    "lookup": (True, False, None, lambda ctx, k: ctx.plonk_prove_gates_lookup(*k.head(), k.desc), "gates_lookup"),
    "zk": (False, True, None, lambda ctx, k: ctx.plonk_prove_gates_zk(*k.head(), NONE, k.blind), "gates_zk"),
    "keccak": (False, False, "keccak", lambda ctx, k: ctx.plonk_prove_gates_h(*k.head(), None, None, "keccak"), "gates_zk"),
    "lookup_zk_keccak": (True, True, "keccak", lambda ctx, k: ctx.plonk_prove_gates_h(*k.head(), k.desc, k.blind, "keccak"), "gates_zk"),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_circuit_data_proves_what_the_matching_direct_entry_proves(ctx, kind):
    import sipp_amd
    lookups, blinded, hasher, entry, size_fn = KINDS[kind]
    k = Case(ctx, lookups, blinded)
    want = entry(ctx, k)
    data = sipp_amd.CircuitData(ctx, k.c.log_n, k.gp, k.fp, k.pc, k.cs, k.c.generators(), sched=k.c.schedule(), digest=bc.PROOF_DIGEST, hasher=hasher)
    try:
        if lookups:
            data.set_lookup(k.desc)
        if blinded:
            data.set_blinding(bc.SEED)                   # counter 0, as k.blind
        got = data.prove(k.c.partial_witness(k.y, A, B), k.pis)
        assert same(got, want), kind
        assert data.verify(got) == (0, 0)
        assert int(ctx.L.sipp_circuit_proof_size(data.h, len(k.pis))) == k.size(ctx.L, size_fn) > 0
    finally:
        data.close()


# entry -> the call with (fri parameters, seed); the two older entries take no seed
ENTRIES = {
    "gates": lambda ctx, k, fp, blind: ctx.plonk_prove_gates(*k.head(fp)),
    "lookup": lambda ctx, k, fp, blind: ctx.plonk_prove_gates_lookup(*k.head(fp), k.desc),
    "zk": lambda ctx, k, fp, blind: ctx.plonk_prove_gates_zk(*k.head(fp), k.desc, blind),
    "h": lambda ctx, k, fp, blind: ctx.plonk_prove_gates_h(*k.head(fp), k.desc, blind, "poseidon"),
}
# (entry, hiding fp, seed) -> the code: a hiding fp without a seed reaches the prover's own check through the two older entries
# (SIPP_E_UNSUPPORTED) and is answered by the two newer ones themselves (SIPP_E_BADARG), as is a seed beside a plain fp
REFUSALS = [("gates", True, False, bc.E_UNSUPPORTED), ("lookup", True, False, bc.E_UNSUPPORTED), ("zk", True, False, bc.E_BADARG),
            ("h", True, False, bc.E_BADARG), ("zk", False, True, bc.E_BADARG), ("h", False, True, bc.E_BADARG)]


def test_each_entry_keeps_its_answer_to_seed_and_hiding_that_disagree(ctx):
    import sipp_amd
    k = Case(ctx, False, False)
    for name, hiding, seeded, code in REFUSALS:
        with pytest.raises(sipp_amd.SippError) as err:
            ENTRIES[name](ctx, k, k.fp_hiding if hiding else k.fp_plain, blinding() if seeded else None)
        assert err.value.code == code, (name, hiding, seeded)
    # the ctx serves the next call
    assert same(ctx.plonk_prove_gates(*k.head()), ctx.plonk_prove_gates_h(*k.head(), None, None, "poseidon"))
