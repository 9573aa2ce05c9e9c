"""The synthetic circuits of tests/_many_generators.py are what tests/test_gpu_witness_many_generators.py takes them for: the generator
counts, the long families at their indices, levels of 5, 3 and 1 rows with copies between them, every generator on a row, and a CPU
replay that writes something for every one of them."""
import numpy as np
import pytest

from sipp_amd.circuit import GEN_COSET_INTERPOLATION, GEN_POSEIDON_SWAP, GEN_REDUCING, GEN_REDUCING_EXT
from tests import _many_generators as mg
from tests import _witness_reading as rd

KIND = {"swap": GEN_POSEIDON_SWAP, "plain": rd.GEN_POSEIDON, "interp": GEN_COSET_INTERPOLATION, "reducing": GEN_REDUCING,
        "reducing_ext": GEN_REDUCING_EXT}


@pytest.mark.parametrize("name", sorted(mg.CIRCUITS))
def test_circuit_is_what_the_gpu_test_takes_it_for(name):
    n_gens, specials = mg.CIRCUITS[name]
    c = mg.ManyGenerators(n_gens, specials)
    gens, sc = c.generators(), c.schedule()
    assert len(gens) == n_gens and c.log_n == 10
    assert len(set(gens)) == n_gens                             # no two generators share kind, selector, gate and parameters
    assert [g[2] for g in gens] == list(range(1, n_gens + 1))   # generator q is gate 1 + q's
    for q, g in enumerate(gens):
        assert (g[0] == KIND[specials[q]]) if q in specials else (g[0] not in KIND.values())
    sizes = list(np.diff(sc["level_offsets"].astype(np.int64)))
    assert sizes == [mg.LEVEL_SIZES[l % 3] for l in range(len(sizes))] and len(sizes) >= 3
    assert all(np.diff(sc["copy_offsets"].astype(np.int64))[:-1] > 0)
    held = np.bincount(c.gate[:c.rows_used], minlength=n_gens + 1)
    assert held[0] == 0 and (held[1:] >= 2).all()
    w, k = c.table(7)
    want = rd.replay(w, k, gens, None, sc)
    changed = (want != w).any(axis=0)
    assert changed[:c.rows_used].all() and not changed[c.rows_used:].any()


def test_33_generators_build_too():
    c = mg.ManyGenerators(33, {32: "swap"})
    assert len(c.generators()) == 33
