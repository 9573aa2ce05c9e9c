"""`xor of two nibbles`: the smallest CircuitBuilder circuit with two tagged lookup tables and a function lookup, for
tests/test_gpu_lookup_tables.py and tests/test_lookup_tables_builder.py.  It says: a and b (witness inputs) are below 16 -- each is
looked up as (v, 0) in a 16-entry range table (tag 1) -- and the public input y is xor4[16 a + b], xor4 the dense 256-entry table
t -> (t >> 4) ^ (t & 15) (tag 0): x = 16 a + b comes from an arithmetic row, y from function_lookup(), whose y cell SIPP_GEN_LOOKUP
fills on the device, and y is tied to the public input, which a Poseidon chain hashes in circuit.  Table rows hold four entries,
looking rows two pairs: the function row is short and repeats its x."""
import numpy as np

from sipp_amd.circuit import _K, _W, P, PUBLIC_INPUT, CircuitBuilder, pi
from sipp_amd.merkle import declare_swap_gate

GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "Arithmetic", "PoseidonSwap", "Table", "Looking"]
GATE_GROUP = (0, 0, 0, 0, 0, 1, 2, 2)
ARITHMETIC, POSEIDON_SWAP, TABLE, LOOKING = 4, 5, 6, 7
GEN_ARITHMETIC = 1                   # include/sipp_hip.h SIPP_GEN_ARITHMETIC
N_LOOK, N_TAB = 2, 4
XOR4 = [(t >> 4) ^ (t & 15) for t in range(256)]


def arithmetic_into(pr, k0, k1):
    """one operation: w3 = c0 w0 w1 + c1 w2"""
    pr.constraint([(1, [(_W, 3)]), (-1, [(_K, k0), (_W, 0), (_W, 1)]), (-1, [(_K, k1), (_W, 2)])])


class XorLookupCircuit(CircuitBuilder):
    n_public_args = 1

    def __init__(self, num_wires=135, num_routed=80, min_log_n=10):
        CircuitBuilder.__init__(self, num_wires, num_routed, GATE_NAMES, GATE_GROUP, 2, 1)
        self.declare_basic(4)
        self.declare(ARITHMETIC, 3, (GEN_ARITHMETIC, 1, self.k0, self.k1), arithmetic_into, self.k0, self.k1)
        declare_swap_gate(self, POSEIDON_SWAP)
        self.declare(TABLE, 0)
        self.declare(LOOKING, 0)
        self.declare_lookup(TABLE, LOOKING, N_LOOK, N_TAB, tables=True)
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        zero, one = self.constant(0)[1], self.constant(1)[1]
        self.xor4 = self.function_table(XOR4)                                   # tag 0
        self.range16 = self.table([(v, 0) for v in range(16)])                  # tag 1
        a, b = self.witness_input(), self.witness_input()
        self.range_check(a, self.range16)
        self.range_check(b, self.range16)
        self.x_row = self.new_row(ARITHMETIC, 16, 1)                            # x = 16 a 1 + 1 b
        self.place(self.x_row, [(0, a), (1, one), (2, b)])
        self.y_cell, = self.function_lookup(self.xor4, [(3, self.x_row)])
        self.tie(pi(0), self.y_cell)
        self.hash_public_inputs(POSEIDON_SWAP, zero)
        self.finish(min_log_n)

    def public_inputs(self, y):
        return [int(y) % P]

    def input_cells(self, y, a, b):
        """(cells, values) of sipp_circuit_prove_inputs: every cell on the cycle of the public input and of the two witness inputs"""
        cells, values = [], []
        for cyc, v in zip(self.pi_cycle + self.in_cycle, (y, a, b)):
            cells += cyc
            values += [int(v) % P] * len(cyc)
        return np.array(cells, dtype=np.uint64), np.array(values, dtype=np.uint64)

    def words_map(self):
        """(cells, sources, n_words, n_extra) of sipp_circuit_set_input_map over the words (y, a, b)"""
        cells, sources = [], []
        for t, cyc in enumerate(self.pi_cycle + self.in_cycle):
            cells += cyc
            sources += [t] * len(cyc)
        return np.array(cells, dtype=np.uint64), np.array(sources, dtype=np.uint64), 3, 0

    def partial_witness(self, y, a, b):
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        cells, values = self.input_cells(y, a, b)
        w.reshape(-1)[cells.astype(np.int64)] = values
        return w
