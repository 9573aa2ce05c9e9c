"""A Python reading of the swap Poseidon row (SIPP_GEN_POSEIDON_SWAP) and of the short families a Merkle-opening circuit uses, as functions
(wires, consts, pih, p, rows) on the rows that hold the generator: the checker of the device witness of sipp_amd/merkle.py.
tests/_witness_reading.py maps the kinds to them and replays a level schedule.

The swap row: s = W(swap); d_i = s (W(in+4+i) - W(in+i)) into W(delta+i); the state (in_i + d_i, in_(4+i) - d_i, in_8 .. in_11) goes through
tools/plonk_synth.poseidon_rows, whose S-box wires are re-based from its own offset to the gate's `sbox`; the outputs are checked against
the oracle's permutation (oracle/poseidon.c) on a sample of rows."""
import os
import sys

import numpy as np

from tests import _oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plonk_synth as ps  # noqa: E402


def poseidon_rows(wires, rows, in_, out, sbox, swap=None, delta=None, check=8):
    """the (swap) Poseidon generator on `rows` of wires [num_wires][N], in place"""
    rows = np.asarray(rows, dtype=np.int64)
    if not len(rows):
        return
    st = np.stack([wires[in_ + i, rows] for i in range(12)])
    if swap is not None:
        s = wires[swap, rows]
        for i in range(4):
            d = ps.gl_mul(s, ps.gl_sub(st[4 + i], st[i]))
            wires[delta + i, rows] = d
            st[i], st[4 + i] = ps.gl_add(st[i], d), ps.gl_sub(st[4 + i], d)
    res, sb = ps.poseidon_rows(st)
    for w, v in sb.items():
        wires[w - ps.POS_SBOX + sbox, rows] = v
    for i in range(12):
        wires[out + i, rows] = res[i]
    for j in range(min(check, len(rows))):               # the permutation itself, against the oracle's
        assert (_oracle.permute(st[:, j]) == np.array([r[j] for r in res], dtype=np.uint64)).all()


def constant_rows(wires, consts, pih, p, rows):
    for l in range(p[0]):
        wires[l, rows] = consts[p[1] + l, rows]


def public_input_rows(wires, consts, pih, p, rows):
    for l in range(4):
        wires[l, rows] = np.uint64(int(pih[l]))


def base_split_rows(wires, consts, pih, p, rows):
    v, mask = wires[0, rows], np.uint64((1 << p[1]) - 1)
    for l in range(p[0]):
        wires[1 + l, rows] = (v >> np.uint64(p[1] * l)) & mask


def random_access_rows(wires, consts, pih, p, rows):
    bits, ln = p[2], 1 << p[2]
    for cp in range(p[0]):
        b = p[1] * cp
        idx = (wires[b, rows] & np.uint64(ln - 1)).astype(np.int64)
        wires[b + 1, rows] = wires[b + 2 + idx, rows]
        for l in range(bits):
            wires[b + 2 + ln + l, rows] = (idx >> l) & 1


def decode(programs, offset, count):
    """program words -> [[(coef mod p, [(kind, index), ...]), ...] per constraint]"""
    out, w = [], offset
    for _ in range(count):
        nm = int(programs[w]); w += 1
        monos = []
        for _m in range(nm):
            coef, nf = int(programs[w]) % _oracle.P, int(programs[w + 1]); w += 2
            monos.append((coef, [(int(programs[w + 2 * f]), int(programs[w + 2 * f + 1])) for f in range(nf)]))
            w += 2 * nf
        out.append(monos)
    return out


def opening(batch, idx, height):
    """(leaves [k][leaf_len], siblings [k][height][4]) of the indices in an _oracle.Batch's tree"""
    leaves = batch.leaves[np.asarray(idx, dtype=np.int64)]
    levels = [batch.level(l) for l in range(height)]
    sib = np.stack([np.stack([levels[l][(int(i) >> l) ^ 1] for l in range(height)]) for i in idx])
    return leaves, sib
