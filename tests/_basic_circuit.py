"""`basic`: the smallest CircuitBuilder circuit with Constant, PublicInput, BaseSum, RandomAccess and arithmetic rows over two selector
columns, for tests that need a circuit and not a statement.  It says: x < 16 (public input 0) splits into four bits; out = a m + (bit 0
of x, 0) over the extension, a and m public inputs 1 .. 4; items[index] of (zero, one, out0, out1) is `claimed`, index a witness
input of two bits.  Public inputs: x, a, m.  Witness inputs: index.  Nothing hashes the public inputs in circuit (no Poseidon gate):
the PublicInput row holds their hash, which the prover binds."""
import numpy as np

from sipp_amd.circuit import (BASE_SUM, GEN_RANDOM_ACCESS, P, PUBLIC_INPUT, CircuitBuilder, pi, random_access_into)
from sipp_amd.fri_fold import EXT_W, arithmetic_row, declare_arithmetic_ext

GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "ArithmeticExt", "RandomAccess"]
ARITHMETIC_EXT, RANDOM_ACCESS = 4, 5
RA_BITS, RA_COPIES = 2, 2
RA_STRIDE = 2 + (1 << RA_BITS) + RA_BITS


class BasicCircuit(CircuitBuilder):
    n_public_args = 1

    def __init__(self, num_wires=135, num_routed=80, min_log_n=10, groups=(0, 0, 0, 0, 1, 1)):
        CircuitBuilder.__init__(self, num_wires, num_routed, GATE_NAMES, groups, 2, 5)
        self.declare_basic(4)
        declare_arithmetic_ext(self, ARITHMETIC_EXT)
        self.declare(RANDOM_ACCESS, RA_BITS + 1, (GEN_RANDOM_ACCESS, RA_COPIES, RA_STRIDE, RA_BITS), random_access_into, RA_COPIES, RA_STRIDE,
                     RA_BITS)
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.zero_row, zero = self.constant(0)
        self.one_row, one = self.constant(1)
        self.split_row = self.new_row(BASE_SUM)
        self.place(self.split_row, [(0, pi(0))])
        bit0 = (1, self.split_row)
        self.arith_row, out = arithmetic_row(self, (pi(1), pi(2)), (pi(3), pi(4)), (bit0, zero), 1, 1)
        self.index = self.witness_input()
        self.ra_row = self.new_row(RANDOM_ACCESS)
        self.place(self.ra_row, [(0, self.index)] + [(2 + j, s) for j, s in enumerate((zero, one) + out)])
        self.finish(min_log_n)

    def declare(self, index, degree, gen=None, fill=None, *args):
        """one selector column has no UNUSED factor: the filter's degree is the number of the other gates, one less than the builder
        counts"""
        return CircuitBuilder.declare(self, index, degree - (self.num_selectors == 1), gen, fill, *args)

    def public_inputs(self, pis):
        assert len(pis) == self.n_pi and 0 <= pis[0] < 16
        return [int(v) % P for v in pis]

    def input_cells(self, pis, index):
        """(cells, values): every cell on the cycle of a public or witness input"""
        cycles, vals = self.pi_cycle + self.in_cycle, self.public_inputs(pis) + [int(index) % 4]
        return (np.array([x for cyc in cycles for x in cyc], dtype=np.uint64),
                np.array([v for cyc, v in zip(cycles, vals) for _ in cyc], dtype=np.uint64))

    def partial_witness(self, pis, index):
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        cells, vals = self.input_cells(pis, index)
        w.reshape(-1)[cells.astype(np.int64)] = vals
        return w

    def expected(self, pis, index):
        """what the rows must hold: (the four bits of x, out, claimed)"""
        x, a0, a1, m0, m1 = self.public_inputs(pis)
        out = ((a0 * m0 + EXT_W * a1 * m1 + (x & 1)) % P, (a0 * m1 + a1 * m0) % P)
        return [(x >> i) & 1 for i in range(4)], out, ((0, 1) + out)[int(index) % 4]
