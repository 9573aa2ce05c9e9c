"""`range check`: the smallest CircuitBuilder circuit with a lookup table, for tests/test_gpu_lookups.py and
tests/test_lookup_builder.py.  It says: every one of the n_values public inputs is below 2^bits -- each is looked up as (x, 0) in the
range table (v, 0), v < 2^bits.  Table rows hold three entries, looking rows four pairs, so the table's last row repeats an entry and
(for n_values no multiple of four) the last looking row repeats its first pair.  Nothing hashes the public inputs in circuit: the
PublicInput row holds their hash, which the prover binds."""
import numpy as np

from sipp_amd.circuit import P, PUBLIC_INPUT, CircuitBuilder, pi

GATE_NAMES = ["Noop", "PublicInput", "Constant", "BaseSum", "Table", "Looking"]
TABLE, LOOKING = 4, 5
N_LOOK, N_TAB = 4, 3


class RangeCheckCircuit(CircuitBuilder):
    n_public_args = 1

    def __init__(self, n_values, bits, num_wires=16, num_routed=12, min_log_n=10):
        CircuitBuilder.__init__(self, num_wires, num_routed, GATE_NAMES, (0, 0, 0, 0, 1, 1), 1, n_values)
        self.declare_basic(4)
        self.declare(TABLE, 0)
        self.declare(LOOKING, 0)
        self.declare_lookup(TABLE, LOOKING, N_LOOK, N_TAB)
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        self.range_table = self.table([(v, 0) for v in range(1 << bits)])
        for t in range(n_values):
            self.range_check(pi(t), self.range_table)
        self.finish(min_log_n)

    def public_inputs(self, values):
        assert len(values) == self.n_pi
        return [int(v) % P for v in values]

    def partial_witness(self, values):
        w = np.zeros((self.num_wires, self.n), dtype=np.uint64)
        flat = w.reshape(-1)
        for cyc, v in zip(self.pi_cycle, self.public_inputs(values)):
            flat[np.asarray(cyc, dtype=np.int64)] = v
        return w
