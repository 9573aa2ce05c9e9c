"""CircuitBuilder's tagged tables and function lookups on the CPU (sipp_amd/circuit.py declare_lookup(tables=True) / table /
function_table / lookup / range_check / function_lookup), on the two-table circuit of tests/_lookup_tables_circuit.py: the constant
columns, the tags, the description, the generator and the levels are what include/sipp_hip.h says; its witness, filled by the integer
reading of SIPP_GEN_LOOKUP, satisfies the tagged reading of the argument.  And with tables=False the builder emits, bit for bit, what
it emitted before it knew of tags."""
import hashlib

import numpy as np
import pytest

from tests import _lookup_tables_cases as tc
from tests._lookup_tables_circuit import ARITHMETIC, LOOKING, N_LOOK, N_TAB, TABLE, XOR4, XorLookupCircuit

P = tc.P


@pytest.fixture(scope="module")
def circ():
    return XorLookupCircuit()


def test_the_description_the_columns_and_the_tags(circ):
    c = circ.circuit()
    q_look, lw, n_look, q_tab, tab0, tm, n_tab, tag0 = c["lookup"]
    assert c["lookup"] == circ.lookup_description() and (n_look, n_tab) == (N_LOOK, N_TAB)
    # behind the selectors: c0, c1, q_look, q_tab, the table columns, the two tag columns
    assert (q_look, q_tab, tab0, tag0) == (circ.k1 + 1, circ.k1 + 2, circ.k1 + 3, circ.k1 + 3 + 2 * n_tab) and tag0 + 2 == c["num_constants"]
    cs = circ.constants_sigmas()
    assert cs.shape == (c["num_constants"] + c["num_routed"], circ.n)
    assert ((cs[q_look] == 1) == (circ.gate == LOOKING)).all() and ((cs[q_tab] == 1) == (circ.gate == TABLE)).all()
    # the handles: tags 0, 1 as the tables came; xor4 dense from its row0
    assert (circ.xor4["tag"], circ.xor4["T"], circ.range16["tag"], circ.range16["T"]) == (0, 256, 1, 16)
    r0, r1 = circ.xor4["row0"], circ.range16["row0"]
    assert r1 == r0 + 64 and (circ.gate[r0:r1 + 4] == TABLE).all() and int(cs[q_tab].sum()) == 68
    for t in (0, 1, 17, 255):
        assert (int(cs[tab0 + 2 * (t % n_tab)][r0 + t // n_tab]), int(cs[tab0 + 2 * (t % n_tab) + 1][r0 + t // n_tab])) == (t, XOR4[t])
    assert [(int(cs[tab0 + 2 * k][r1 + 3]), int(cs[tab0 + 2 * k + 1][r1 + 3])) for k in range(n_tab)] == [(v, 0) for v in range(12, 16)]
    assert (cs[tag0 + 1][r0:r1] == 0).all() and (cs[tag0 + 1][r1:r1 + 4] == 1).all()
    # two looking rows: the range checks of a and b under tag 1 with c0 = c1 = 0, the function row under tag 0 with c0 = row0, c1 = T
    rng_row, fn_row = [int(r) for r in np.flatnonzero(circ.gate == LOOKING)]
    assert fn_row == circ.y_cell[1] and circ.y_cell[0] == lw + 1
    assert (int(cs[tag0][rng_row]), int(cs[circ.k0][rng_row]), int(cs[circ.k1][rng_row])) == (1, 0, 0)
    assert (int(cs[tag0][fn_row]), int(cs[circ.k0][fn_row]), int(cs[circ.k1][fn_row])) == (0, r0, 256)


def test_the_generator_and_the_levels(circ):
    q_look, lw, n_look, q_tab, tab0, tm, n_tab, tag0 = circ.lookup_description()
    gens = [g for g in circ.generators() if g[0] == tc.GEN_LOOKUP]
    assert gens == [(tc.GEN_LOOKUP, 2, LOOKING, lw, n_look, tab0, n_tab, circ.k0)]
    lv = circ.row_level
    rng_row, fn_row = [int(r) for r in np.flatnonzero(circ.gate == LOOKING)]
    assert lv[circ.x_row] == 1 and lv[fn_row] == lv[circ.x_row] + 1 and lv[rng_row] == 1 and circ.n_levels == 3
    # the function row's x cells are copied from the arithmetic row's output at that row's level; its y cells are nobody's copy
    n = circ.n
    sc = circ.schedule()
    into = {int(d): int(s) for s, d in zip(sc["copy_src"], sc["copy_dst"])}
    assert into[lw * n + fn_row] == 3 * n + circ.x_row and into[(lw + 2) * n + fn_row] == 3 * n + circ.x_row
    assert (lw + 1) * n + fn_row not in into and (lw + 3) * n + fn_row not in into
    # y is on the public input's cycle, with the cell the hash chain absorbs
    assert circ.pi_cycle == [sorted([(lw + 1) * n + fn_row, circ.s_in * n + circ.chain_row[0]])]
    assert circ.gate[circ.x_row] == ARITHMETIC


def witness(circ, y, a, b):
    """the looking rows' witness without the device: the inputs, x = 16 a + b by hand, the copies into the function row, then the
    integer reading of the generator on the circuit's own constants"""
    q_look, lw, n_look, q_tab, tab0, tm, n_tab, tag0 = circ.lookup_description()
    consts = circ.constants_sigmas()[:circ.num_constants]
    w = circ.partial_witness(y, a, b)
    fn_row = circ.y_cell[1]
    w[3][circ.x_row] = (16 * a + b) % P
    w[lw][fn_row] = w[lw + 2][fn_row] = w[3][circ.x_row]
    w, _ = tc.generate(w, consts, [g for g in circ.generators() if g[0] == tc.GEN_LOOKUP])
    return w, consts


def test_the_witness_satisfies_the_tagged_reading(circ):
    desc = circ.lookup_description()
    w, consts = witness(circ, 5, 9, 12)
    fn_row = circ.y_cell[1]
    assert int(w[circ.y_cell[0]][fn_row]) == XOR4[0x9c] == 5 and int(w[desc[1] + 3][fn_row]) == 5
    full = tc.multiplicities(desc, w, consts)
    assert int(full[desc[5]: desc[5] + N_TAB].sum()) == 2 * N_LOOK
    e = dict(desc=desc, consts=consts, D=8, C=2, log_n=circ.log_n, etas=[5, 1 << 40], thetas=[P - 3, 77])
    cols, closes = tc.sums(desc, full, consts, 8, e["etas"], e["thetas"])
    assert closes and tc.all_terms_vanish(e, full, cols)
    # a = 16: x = 268 is outside xor4 and the generator writes y = 0; (16, 0) is no entry of the range table, (268, 0) none of xor4
    bad, _ = witness(circ, 0, 16, 12)
    assert int(bad[circ.y_cell[0]][fn_row]) == 0
    with pytest.raises(tc.Absent):
        tc.multiplicities(desc, bad, consts)


def test_without_tables_the_builder_emits_what_it_emitted():
    """the digest of everything RangeCheckCircuit hands the prover, recorded from the builder before it knew of tags"""
    from tests._lookup_circuit import RangeCheckCircuit
    c = RangeCheckCircuit(n_values=11, bits=5)
    sc = c.schedule()
    parts = [c.constants_sigmas(), c.programs, np.array(c.generators(), dtype=np.int64), np.array(c.lookup_description(), dtype=np.int64),
             np.array(c.gates, dtype=np.int64), sc["rows"], sc["level_offsets"], sc["copy_src"], sc["copy_dst"], sc["copy_offsets"], sc["row_level"],
             c.partial_witness(list(range(c.n_pi)))]
    h = hashlib.sha256()
    for a in parts:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    assert h.hexdigest() == "4788d8636b49e3c5f4d7978bb7a354f452d546fca551c8f39c1c0b1d8337c531"
    assert c.lookup_description()[7] == 0 and all(g[0] != tc.GEN_LOOKUP for g in c.generators())


def test_the_builder_refuses_what_the_layout_cannot_hold():
    from sipp_amd.circuit import CircuitBuilder
    b = CircuitBuilder(16, 12, ["Noop", "PublicInput", "Constant", "BaseSum", "Table", "Looking"], (0, 0, 0, 0, 1, 1), 1, 1)
    b.declare_basic(4)
    b.declare(TABLE - 2, 0)
    b.declare(LOOKING - 2, 0)
    with pytest.raises(AssertionError):              # one constant column: nowhere to keep row0 and T
        b.declare_lookup(TABLE - 2, LOOKING - 2, 2, 2, tables=True)


def test_the_recursion_circuits_refuse_an_inner_circuit_with_tagged_lookups(circ):
    from sipp_amd.plonk_vanishing import PlonkVanishingCircuit
    with pytest.raises(AssertionError, match="lookups"):
        PlonkVanishingCircuit(circ.log_n, (circ.num_routed, 8, 2), circ.circuit(), 4, 1)
