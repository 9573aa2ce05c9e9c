"""CircuitBuilder's lookups on the CPU (sipp_amd/circuit.py declare_lookup / table / lookup / range_check): the description and the
constant columns a range-check circuit emits, read by the Python-integer reading of tests/_lookup_cases.py -- the multiplicities of its
witness make every term of the argument vanish, a value outside the table is found absent -- and a builder that declares no table
emits the circuit it emitted before."""
import numpy as np
import pytest

from tests import _lookup_cases as lc
from tests._lookup_circuit import LOOKING, N_LOOK, N_TAB, TABLE, RangeCheckCircuit

VALUES = [3, 31, 0, 7, 7, 7, 30, 1, 2, 16, 15]


@pytest.fixture(scope="module")
def circ():
    return RangeCheckCircuit(n_values=len(VALUES), bits=5)


def test_the_description_rides_in_the_circuit_and_fits_it(circ):
    c = circ.circuit()
    q_look, lw, n_look, q_tab, tc, tm, n_tab, last = c["lookup"]
    assert c["lookup"] == circ.lookup_description() and (n_look, n_tab, last) == (N_LOOK, N_TAB, 0)
    assert c["num_selectors"] <= q_look < q_tab < tc and tc + 2 * n_tab == c["num_constants"]
    assert lw + 2 * n_look <= c["num_routed"] and tm + n_tab <= c["num_wires"]
    assert c["gates"][TABLE][5] == 0 and c["gates"][LOOKING][5] == 0            # bookkeeping gates: no constraints
    cs = circ.constants_sigmas()
    assert cs.shape == (c["num_constants"] + c["num_routed"], circ.n)
    assert ((cs[q_look] == 1) == (circ.gate == LOOKING)).all() and ((cs[q_tab] == 1) == (circ.gate == TABLE)).all()
    assert set(np.unique(cs[q_look])) <= {0, 1} and set(np.unique(cs[q_tab])) <= {0, 1}
    assert int(cs[q_look].sum()) == -(-len(VALUES) // N_LOOK) and int(cs[q_tab].sum()) == -(-32 // N_TAB)
    # the table's entries, row by row; the last row's spare slot repeats the last entry
    rows = np.flatnonzero(cs[q_tab])
    got = [(int(cs[tc + 2 * k][r]), int(cs[tc + 2 * k + 1][r])) for r in rows for k in range(n_tab)]
    assert got == [(v, 0) for v in range(32)] + [(31, 0)]


def test_the_witness_satisfies_the_reading_and_a_value_outside_is_absent(circ):
    desc = circ.lookup_description()
    K = circ.num_constants
    consts = circ.constants_sigmas()[:K]
    wires = circ.partial_witness(VALUES)        # the y wires copy a Constant row's 0: the partial witness is the looking rows' witness
    full = lc.multiplicities(desc, wires, consts)
    tm = desc[5]
    assert int(full[tm: tm + N_TAB].sum()) == N_LOOK * -(-len(VALUES) // N_LOOK)         # the short last row repeats its first pair
    e = dict(desc=desc, consts=consts, D=8, C=2, log_n=circ.log_n, etas=[5, 1 << 40], thetas=[lc.P - 3, 77])
    cols, closes = lc.sums(desc, full, consts, 8, e["etas"], e["thetas"])
    assert closes and lc.all_terms_vanish(e, full, cols)
    with pytest.raises(lc.Absent):
        lc.multiplicities(desc, circ.partial_witness(VALUES[:-1] + [32]), consts)


def test_a_builder_without_a_table_emits_what_it_emitted():
    from tests._basic_circuit import BasicCircuit
    b = BasicCircuit()
    assert "lookup" not in b.circuit() and b.lookup_description() == (0,) * 8
    assert b.num_constants == b.num_selectors + 2 and b.constants_sigmas().shape[0] == b.num_constants + b.num_routed


def test_the_recursion_circuits_refuse_an_inner_circuit_with_lookups(circ):
    from sipp_amd.plonk_vanishing import PlonkVanishingCircuit
    with pytest.raises(AssertionError, match="lookups"):
        PlonkVanishingCircuit(circ.log_n, (circ.num_routed, 8, 2), circ.circuit(), 4, len(VALUES))
