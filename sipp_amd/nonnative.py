"""u32 and nonnative arithmetic in the outer circuit: plonky2_u32's U32ArithmeticGate and U32AddManyGate AS RECALLED (the crates are not
vendored; the wire layouts are this library's, INTEGRATION.md states them), the BigUint gadgets built on them, and reduce / inverse of a
256-bit value modulo a modulus that is data.  The generators are SIPP_GEN_U32_ARITHMETIC, _U32_ADD_MANY and _NONNATIVE (include/sipp_hip.h).

  u32_range_into, u32_arithmetic_into, u32_add_many_into    the gate programs, degree 4
  NonnativeBuilder          a CircuitBuilder with the gadgets: range_check_u32, u32_products, add_many, mul_biguint, add_biguint,
                            less_than_constant, reduce, inverse

The u32 arithmetic gate, per op at b = ARITH_STRIDE k: a, b, c, lo, hi, the inverse cell, sixteen 2-bit limbs of lo, sixteen of hi:
    a b + c - lo - 2^32 hi = 0        (inverse (2^32 - 1 - hi) - 1) lo = 0        lo, hi = their limbs' sums        every limb in 0 .. 3
With a, b, c u32 (range-checked where they were made) the integer a b + c is at most (2^32 - 1)^2 + 2^32 - 1 = p - 1, and lo + 2^32 hi
< 2^64 equals it mod p: as an integer it is that value V or V + p.  The second constraint forces lo = 0 where hi = 2^32 - 1, so
lo + 2^32 hi <= p - 1 and the split is V's.  (A fourth operand would let V reach p: the gate has none.)
The add-many gate, per op: sixteen addends, the carry-in, lo, the carry-out, sixteen 2-bit limbs of lo, three of the carry-out:
    sum + carry-in - lo - 2^32 carry-out = 0, both sides far below p: the equation holds in integers.
A u32 range check is a row of its own (U32Range: the value and its sixteen 2-bit limbs, generator SIPP_GEN_BASE_SPLIT).

Soundness of reduce(x, m) -> rem, in integers: the generator writes rem, q and slack; all 24 limbs are range-checked; q m + rem is
computed limb by limb (64 products, 16 column sums chained by their carries, rem the extra addend of columns 0 .. 7) and tied to x's
eight limbs, to zero above them, the top carry to zero: x = q m + rem; rem + slack + 1 = m limb by limb with the top carry zero: rem < m.
inverse(x, m) -> inv: inv, k and slack range-checked; x inv and k m + 1 computed over sixteen limbs and tied limb for limb, both top
carries zero: x inv = k m + 1; inv + slack + 1 = m: inv < m.  rem and inv are therefore THE values, not merely congruent ones.

numpy only; imports nothing from the test oracle."""
from .circuit import GEN_BASE_SPLIT, GEN_NONNATIVE, GEN_U32_ADD_MANY, GEN_U32_ARITHMETIC, CircuitBuilder, _W

M32 = 0xFFFFFFFF
LIMBS = 16                                                      # 2-bit limbs of a u32
ARITH_OPS, ARITH_STRIDE = 2, 6 + 2 * LIMBS                      # a, b, c, lo, hi, inverse, the limbs: 38 wires an op
ADD_ADDENDS, ADD_CARRY_LIMBS = 16, 3                            # the widest column of an 8 x 8 limb product (15) and one more addend
ADD_OPS, ADD_STRIDE = 1, ADD_ADDENDS + 3 + LIMBS + ADD_CARRY_LIMBS
NN_X, NN_M, NN_OUT = 0, 8, 16                                   # a nonnative row: x, m, then result, quotient, slack


def _two_bit(pr, w):
    """x (x - 1) (x - 2) (x - 3)"""
    x = (_W, w)
    pr.constraint([(1, [x] * 4), (-6, [x] * 3), (11, [x] * 2), (-6, [x])])


def _limb_sum(pr, value, first, n_limbs):
    pr.constraint([(1 << (2 * l), [(_W, first + l)]) for l in range(n_limbs)] + [(-1, [(_W, value)])])


def u32_range_into(pr):
    _limb_sum(pr, 0, 1, LIMBS)
    for l in range(LIMBS):
        _two_bit(pr, 1 + l)


def u32_arithmetic_into(pr, n_ops, stride, n_limbs):
    for op in range(n_ops):
        b = stride * op
        a, bb, c, lo, hi, inv = [(_W, b + t) for t in range(6)]
        pr.constraint([(1, [a, bb]), (1, [c]), (-1, [lo]), (-(1 << 32), [hi])])
        pr.constraint([(M32, [inv, lo]), (-1, [inv, hi, lo]), (-1, [lo])])
        _limb_sum(pr, b + 3, b + 6, n_limbs)
        _limb_sum(pr, b + 4, b + 6 + n_limbs, n_limbs)
        for l in range(2 * n_limbs):
            _two_bit(pr, b + 6 + l)


def u32_add_many_into(pr, n_ops, stride, n_addends, n_carry_limbs):
    for op in range(n_ops):
        b = stride * op
        lo, carry = b + n_addends + 1, b + n_addends + 2
        pr.constraint([(1, [(_W, b + t)]) for t in range(n_addends + 1)] + [(-1, [(_W, lo)]), (-(1 << 32), [(_W, carry)])])
        _limb_sum(pr, lo, b + n_addends + 3, LIMBS)
        _limb_sum(pr, carry, b + n_addends + 3 + LIMBS, n_carry_limbs)
        for l in range(LIMBS + n_carry_limbs):
            _two_bit(pr, b + n_addends + 3 + l)


class NonnativeBuilder(CircuitBuilder):
    """CircuitBuilder with the u32 / BigUint / nonnative gadgets.  A value is a list of limb sources, least significant first; every
    gadget returns cells.  declare_nonnative() names the five gates; `zero` and `one` are the constants' cells."""

    def declare_nonnative(self, range_gate, arith_gate, add_gate, reduce_gate, inverse_gate):
        assert ARITH_OPS * ARITH_STRIDE <= self.num_wires and ARITH_STRIDE * (ARITH_OPS - 1) + 5 <= self.num_routed
        assert ADD_STRIDE <= self.num_wires and NN_OUT + 24 <= self.num_routed
        self.g_range, self.g_arith, self.g_add, self.g_reduce, self.g_inverse = range_gate, arith_gate, add_gate, reduce_gate, inverse_gate
        gens = {range_gate: (4, (GEN_BASE_SPLIT, LIMBS, 2), u32_range_into, ()),
                arith_gate: (4, (GEN_U32_ARITHMETIC, ARITH_OPS, ARITH_STRIDE, LIMBS), u32_arithmetic_into, (ARITH_OPS, ARITH_STRIDE, LIMBS)),
                add_gate: (4, (GEN_U32_ADD_MANY, ADD_OPS, ADD_STRIDE, ADD_ADDENDS, ADD_CARRY_LIMBS), u32_add_many_into,
                           (ADD_OPS, ADD_STRIDE, ADD_ADDENDS, ADD_CARRY_LIMBS)),
                reduce_gate: (0, (GEN_NONNATIVE, 0, NN_X, NN_M, NN_OUT), None, ()),
                inverse_gate: (0, (GEN_NONNATIVE, 1, NN_X, NN_M, NN_OUT), None, ())}
        for index in sorted(gens):
            degree, gen, fill, args = gens[index]
            self.declare(index, degree, gen, fill, *args)
        self.u32_rows = {"range": [], "arith": [], "add": [], "reduce": [], "inverse": []}

    def set_constants(self, zero, one):
        self.nn_zero, self.nn_one = zero, one

    def range_check_u32(self, source):
        r = self.new_row(self.g_range)
        self.place(r, [(0, source)])
        self.u32_rows["range"].append(r)
        return r

    def u32_products(self, ops):
        """ops = [(a, b, c)] of u32 sources -> [(lo, hi)] of a b + c, ARITH_OPS to a row; a short row's other ops are 0 0 + 0"""
        out = []
        for at in range(0, len(ops), ARITH_OPS):
            chunk = list(ops[at:at + ARITH_OPS])
            r = self.new_row(self.g_arith)
            feeds = []
            for k in range(ARITH_OPS):
                a, b, c = chunk[k] if k < len(chunk) else (self.nn_zero,) * 3
                feeds += [(ARITH_STRIDE * k, a), (ARITH_STRIDE * k + 1, b), (ARITH_STRIDE * k + 2, c)]
            self.place(r, feeds)
            self.u32_rows["arith"].append(r)
            out += [((ARITH_STRIDE * k + 3, r), (ARITH_STRIDE * k + 4, r)) for k in range(len(chunk))]
        return out

    def add_many(self, addends, carry_in):
        """up to ADD_ADDENDS u32 sources and a carry-in -> (lo, carry-out)"""
        assert 1 <= len(addends) <= ADD_ADDENDS
        r = self.new_row(self.g_add)
        self.place(r, [(t, addends[t] if t < len(addends) else self.nn_zero) for t in range(ADD_ADDENDS)] + [(ADD_ADDENDS, carry_in)])
        self.u32_rows["add"].append(r)
        return (ADD_ADDENDS + 1, r), (ADD_ADDENDS + 2, r)

    def mul_biguint(self, a, b, addend=None):
        """a b + addend over len(a) + len(b) limbs (a, b of up to eight limbs, addend of at most that many): the products side by side,
        then the column sums chained by their carries -- len(a) + len(b) + 1 levels -> (limbs, the top carry: zero in integers)"""
        assert len(a) <= 8 and len(b) <= 8
        pairs = [(i, j) for i in range(len(a)) for j in range(len(b))]
        prod = dict(zip(pairs, self.u32_products([(a[i], b[j], self.nn_zero) for i, j in pairs])))
        limbs, carry = [], self.nn_zero
        for k in range(len(a) + len(b)):
            col = [prod[p][0] for p in pairs if sum(p) == k] + [prod[p][1] for p in pairs if sum(p) == k - 1]
            if addend is not None and k < len(addend):
                col.append(addend[k])
            lo, carry = self.add_many(col, carry)
            limbs.append(lo)
        return limbs, carry

    def add_biguint(self, a, b, extra=None):
        """a + b (+ extra, a single u32 source, into limb 0) limb by limb, chained by the carries -> (limbs, the top carry)"""
        assert len(a) == len(b)
        limbs, carry = [], self.nn_zero
        for k in range(len(a)):
            lo, carry = self.add_many([a[k], b[k]] + ([extra] if extra is not None and k == 0 else []), carry)
            limbs.append(lo)
        return limbs, carry

    def less_than_constant(self, x, slack, bound):
        """x < bound: x + slack + 1 = bound limb for limb with no top carry, slack range-checked by the caller; bound: cells (constants)"""
        limbs, carry = self.add_biguint(x, slack, self.nn_one)
        for k, c in enumerate(limbs):
            self.tie(c, bound[k])
        self.tie(carry, self.nn_zero)

    def _nonnative_row(self, gate, name, x, modulus):
        assert len(x) == 8 and len(modulus) == 8
        r = self.new_row(gate)
        self.place(r, [(NN_X + k, x[k]) for k in range(8)] + [(NN_M + k, modulus[k]) for k in range(8)])
        self.u32_rows[name].append(r)
        out = [[(NN_OUT + 8 * part + k, r) for k in range(8)] for part in range(3)]
        for part in out:
            for c in part:
                self.range_check_u32(c)
        return out

    def reduce(self, limbs, modulus):
        """eight u32 limb sources, the modulus' eight constant cells -> the limbs of x mod m (generated, range-checked, below m)"""
        rem, q, slack = self._nonnative_row(self.g_reduce, "reduce", limbs, modulus)
        total, carry = self.mul_biguint(q, modulus, rem)
        for k, c in enumerate(total):
            self.tie(c, limbs[k] if k < 8 else self.nn_zero)
        self.tie(carry, self.nn_zero)
        self.less_than_constant(rem, slack, modulus)
        return rem

    def inverse(self, limbs, modulus):
        """-> the limbs of (x mod m)^-1 mod m; no witness exists where there is no inverse"""
        inv, k, slack = self._nonnative_row(self.g_inverse, "inverse", limbs, modulus)
        left, c1 = self.mul_biguint(limbs, inv)
        right, c2 = self.mul_biguint(k, modulus, [self.nn_one])
        for l, r in zip(left, right):
            self.tie(l, r)
        self.tie(c1, self.nn_zero)
        self.tie(c2, self.nn_zero)
        self.less_than_constant(inv, slack, modulus)
        return inv
