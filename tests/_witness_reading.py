"""The one Python reading of the outer prover's witness generators: the SIPP_GEN_* numbers, a table from a generator's kind to the
function that reads its family on the rows that hold it, and the CPU forms of the two entry points (sipp_plonk_generate_witness_levels:
replay, sipp_plonk_generate_witness: row_local).  The families themselves are read where they were first needed: the Poseidon rows and
the short families in tests/_merkle_reading.py, the fold chain's in tests/_fri_fold_reading.py, the initial combination's in
tests/_fri_initial_reading.py.  A test compares the families it hands over and no others: a held row of an unread kind (1, 5) is an
error, not a skipped row."""
import numpy as np

from sipp_amd.circuit import (GEN_ARITHMETIC_EXT, GEN_BASE_SPLIT, GEN_CONSTANT, GEN_COSET_INTERPOLATION, GEN_EXPONENTIATION,
                              GEN_POSEIDON_SWAP, GEN_PUBLIC_INPUT, GEN_QUOTIENT_EXT, GEN_RANDOM_ACCESS, GEN_REDUCING, GEN_REDUCING_EXT)
from tests import _fri_fold_reading as fr
from tests import _fri_initial_reading as ir
from tests import _merkle_reading as mr
from tests._merkle_reading import ps

GEN_ARITHMETIC, GEN_U32_MUL_ADD, GEN_POSEIDON = ps.GEN_ARITHMETIC, ps.GEN_U32_MUL_ADD, ps.GEN_POSEIDON


def _row_by_row(row):
    """a family read in exact integers: row(w, p, c) on one row's wires as a list of ints, in place; c(j) = the row's constant j"""
    def on_rows(wires, consts, pih, p, rows):
        for r in rows:
            w = [int(x) for x in wires[:, r]]
            row(w, p, lambda j: int(consts[j, r]))
            wires[:, r] = np.array(w, dtype=np.uint64)
    return on_rows


# kind -> f(wires, consts, pih, p, rows): the generator with parameters p = (p0 .. p4) on `rows`, all of which hold it, in place
READINGS = {
    GEN_POSEIDON: lambda wires, consts, pih, p, rows: mr.poseidon_rows(wires, rows, p[0], p[1], p[2]),
    GEN_POSEIDON_SWAP: lambda wires, consts, pih, p, rows: mr.poseidon_rows(wires, rows, p[0], p[1], p[2], swap=p[3], delta=p[4]),
    GEN_CONSTANT: mr.constant_rows,
    GEN_PUBLIC_INPUT: mr.public_input_rows,
    GEN_BASE_SPLIT: mr.base_split_rows,
    GEN_RANDOM_ACCESS: mr.random_access_rows,
    GEN_ARITHMETIC_EXT: _row_by_row(lambda w, p, c: fr.arithmetic_ext_row(w, c(p[1]), c(p[2]), p[0], p[3])),
    GEN_EXPONENTIATION: _row_by_row(lambda w, p, c: fr.exponentiation_row(w, p[0])),
    GEN_COSET_INTERPOLATION: _row_by_row(lambda w, p, c: fr.coset_interpolation_row(w, p[0], p[1], p[2])),
    GEN_REDUCING: _row_by_row(lambda w, p, c: ir.reducing_row(w, p[0], p[1])),
    GEN_REDUCING_EXT: _row_by_row(lambda w, p, c: ir.reducing_ext_row(w, p[0], p[1])),
    GEN_QUOTIENT_EXT: _row_by_row(lambda w, p, c: ir.quotient_ext_row(w, c(p[1]), c(p[2]), p[0], p[3])),
}


def run_generator(wires, consts, pih, g, rows):
    """one generator (kind, selector_index, row, p0 .. p4) on the given rows whose selector cell holds its gate index"""
    kind, si, gate, p = g[0], g[1], g[2], g[3:8]
    rows = np.asarray(rows, dtype=np.int64)
    rows = rows[consts[si, rows] == np.uint64(gate)]
    if not len(rows):
        return
    if kind not in READINGS:
        raise ValueError("no reading of generator kind %d" % kind)
    READINGS[kind](wires, consts, pih, p, rows)


def replay(wires, consts, gens, pih, sched):
    """sipp_plonk_generate_witness_levels on the CPU: per level the generators of its rows, then the copies its outputs feed"""
    w = np.ascontiguousarray(wires, dtype=np.uint64).copy()
    flat = w.reshape(-1)
    rows, lo, co = sched["rows"].astype(np.int64), sched["level_offsets"], sched["copy_offsets"]
    src, dst = sched["copy_src"].astype(np.int64), sched["copy_dst"].astype(np.int64)
    for lv in range(int(sched["n_levels"])):
        r = rows[lo[lv]:lo[lv + 1]]
        for g in gens:
            run_generator(w, consts, pih, g, r)
        flat[dst[co[lv]:co[lv + 1]]] = flat[src[co[lv]:co[lv + 1]]]
    return w


def row_local(wires, consts, gens, pih):
    """sipp_plonk_generate_witness on the CPU: every generator on every row of its gate"""
    w = np.ascontiguousarray(wires, dtype=np.uint64).copy()
    for g in gens:
        run_generator(w, consts, pih, g, np.arange(w.shape[1]))
    return w
