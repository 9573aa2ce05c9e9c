"""Synthetic circuits with many witness generators, on sipp_amd.circuit.CircuitBuilder: what tests/test_gpu_witness_many_generators.py runs
through sipp_plonk_generate_witness_levels at and past the sixteen generators the level kernels' narrow argument struct carries.

A circuit has n_gens gates with a generator behind Noop.  `specials` puts the long families at chosen generator indices: "swap"
(SIPP_GEN_POSEIDON_SWAP), "plain" (SIPP_GEN_POSEIDON), "interp" (SIPP_GEN_COSET_INTERPOLATION, 16 points, degree 7), "reducing" and
"reducing_ext" (19 coefficients).  Every other index holds a cheap gate of parameters of its own: Constant, BaseSplit and BaseSum with
2 .. 17 one-bit limbs.  The selector groups are filled greedily so that CircuitBuilder.declare's assertion (gates in the group plus the
gate's degree at most 8) admits every gate.

The rows come in levels of 5, 3 and 1 (so the sixteen-lane kernels' groups of four are not full) until every gate has held two rows; a row
behind level 0 takes one input from an output cell of the level before, so every level ends in copies.  `wide_level` puts 16384 rows
in front as level 0 of a 2^15 table: the one-lane-per-row kernel.  The wire table is random field values (every family takes any value
in its inputs; a swap row's swap wire holds 0 or 1): the generators overwrite what is theirs, everything else must come back as it was."""
import numpy as np

from sipp_amd.circuit import (GEN_BASE_SPLIT, GEN_BASE_SUM, GEN_CONSTANT, GEN_COSET_INTERPOLATION, GEN_REDUCING, GEN_REDUCING_EXT, P,
                              CircuitBuilder, base_sum_into, constant_into)
from sipp_amd.fri_fold import EXT_W, INTERP_DEGREE, coset_interpolation_into, interpolation_layout
from sipp_amd.fri_initial import _reducing_into, reducing_layout
from sipp_amd.merkle import declare_swap_gate
from tests import _challenger_reading  # noqa: F401  (registers the reading of SIPP_GEN_BASE_SUM)
from tests import _witness_reading as rd

NUM_WIRES, NUM_ROUTED = 135, 80
K_REDUCING = 19
INTERP_BITS = 4
LEVEL_SIZES = (5, 3, 1)
WIDE_ROWS = 16384                                               # witness.hip COOP_BELOW_ROWS: a level of this many rows takes one lane per row


def _gates(n_gens, specials):
    """per generator index (name, degree, declare(b, index), input wire, output wire)"""
    il, rl, xl = interpolation_layout(INTERP_BITS, INTERP_DEGREE), reducing_layout(K_REDUCING, False), reducing_layout(K_REDUCING, True)
    special = {
        "swap": (7, lambda b, i: declare_swap_gate(b, i), 1, 12),
        # upstream's PoseidonGate without its swap: the generator alone, no program (only witness generation runs these circuits)
        "plain": (7, lambda b, i: b.declare(i, 7, (rd.GEN_POSEIDON, b.s_in, b.s_out, b.s_sbox)), 1, 12),
        "interp": (INTERP_DEGREE, lambda b, i: b.declare(i, INTERP_DEGREE, (GEN_COSET_INTERPOLATION, INTERP_BITS, INTERP_DEGREE, EXT_W),
                                                         coset_interpolation_into, INTERP_BITS, INTERP_DEGREE, EXT_W), il["values"], il["eval"]),
        "reducing": (2, lambda b, i: b.declare(i, 2, (GEN_REDUCING, K_REDUCING, EXT_W), _reducing_into, K_REDUCING, EXT_W, False),
                     rl["coeffs"], rl["last"]),
        "reducing_ext": (2, lambda b, i: b.declare(i, 2, (GEN_REDUCING_EXT, K_REDUCING, EXT_W), _reducing_into, K_REDUCING, EXT_W, True),
                         xl["coeffs"], xl["last"]),
    }
    cheap = [("Constant", 1, lambda b, i: b.declare(i, 1, (GEN_CONSTANT, 1, b.k0), constant_into, b.k0), 5, 0)]
    for nb in range(2, 18):
        cheap.append(("BaseSplit%d" % nb, 2, lambda b, i, nb=nb: b.declare(i, 2, (GEN_BASE_SPLIT, nb, 1), base_sum_into, nb), 0, 1))
        cheap.append(("BaseSum%d" % nb, 2, lambda b, i, nb=nb: b.declare(i, 2, (GEN_BASE_SUM, nb, 1), base_sum_into, nb), 1, 0))
    out, it = [], iter(cheap)
    for q in range(n_gens):
        if q in specials:
            out.append((specials[q],) + special[specials[q]])
        else:
            out.append(next(it))
    return out


def _groups(degrees):
    """the selector group of every gate, filled greedily: gates in the group + the largest degree among them <= 8"""
    groups, size, top = [], 0, 0
    for d in degrees:
        if size and size + 1 + max(top, d) > 8:
            groups.append(groups[-1] + 1)
            size, top = 1, d
        else:
            groups.append(groups[-1] if groups else 0)
            size, top = size + 1, max(top, d)
    return tuple(groups)


class ManyGenerators(CircuitBuilder):
    def __init__(self, n_gens, specials, wide_level=False):
        assert all(0 <= q < n_gens for q in specials)
        gates = _gates(n_gens, specials)
        names = ["Noop"] + ["%s@%d" % (g[0], q) for q, g in enumerate(gates)]
        CircuitBuilder.__init__(self, NUM_WIRES, NUM_ROUTED, names, _groups([0] + [g[1] for g in gates]), 2, 0)
        self.declare(0, 0)
        for q, g in enumerate(gates):
            g[2](self, 1 + q)
        self.swap_rows, rng = [], np.random.default_rng(1600 + n_gens)
        at, before = 0, []                                      # the next gate; the rows of the level before

        def row(feeds):
            nonlocal at
            q = at % n_gens
            at += 1
            r = self.new_row(1 + q, int(rng.integers(0, P, dtype=np.uint64)))
            self.place(r, [(gates[q][3], s) for s in feeds])
            if gates[q][0] == "swap":
                self.swap_rows.append(r)
            return (gates[q][4], r)
        if wide_level:
            before = [row([]) for _ in range(WIDE_ROWS)]
        lv = 0
        while at < 2 * n_gens + (WIDE_ROWS if wide_level else 0):
            size = LEVEL_SIZES[lv % 3]
            before = [row([before[(7 * k) % len(before)]] if before else []) for k in range(size)]
            lv += 1
        self.finish(15 if wide_level else 10)

    def table(self, seed):
        """(wires, constants): random field values; 0 or 1 in the swap wire of the swap rows"""
        rng = np.random.default_rng(seed)
        w = rng.integers(0, P, (NUM_WIRES, self.n), dtype=np.uint64)
        for r in self.swap_rows:
            w[self.s_swap, r] = r & 1
        return w, np.ascontiguousarray(self.constants_sigmas()[:self.num_constants])


# name -> (n_gens, specials): 16 is the narrow struct's last size; 17 puts every long family in turn at index 16, and picks each
# sixteen-lane kernel of the wide width (swap alone: <false, false>; with an interpolation: <true, false>; with the reducing
# families: <true, true>; one plain Poseidon generator and no swap: plonk_witness_level_coop_kernel)
CIRCUITS = {
    "16": (16, {12: "interp", 13: "reducing", 14: "reducing_ext", 15: "swap"}),
    "17-swap-at-16": (17, {13: "interp", 14: "reducing", 15: "reducing_ext", 16: "swap"}),
    "17-interp-at-16": (17, {13: "reducing", 14: "reducing_ext", 15: "swap", 16: "interp"}),
    "17-reducing-at-16": (17, {13: "reducing_ext", 14: "swap", 15: "interp", 16: "reducing"}),
    "17-reducing-ext-at-16": (17, {13: "swap", 14: "interp", 15: "reducing", 16: "reducing_ext"}),
    "17-swap-alone": (17, {16: "swap"}),
    "17-swap-and-interp": (17, {3: "swap", 16: "interp"}),
    "17-plain-at-16": (17, {16: "plain"}),
    "17-plain-at-0": (17, {0: "plain"}),
    "31": (31, {16: "swap", 20: "interp", 27: "reducing", 30: "reducing_ext"}),
    "32": (32, {28: "interp", 29: "reducing", 30: "reducing_ext", 31: "swap"}),
    "32-spread": (32, {16: "reducing_ext", 17: "interp", 24: "swap", 31: "reducing"}),
}
