"""A Python reading of the swap Poseidon row (SIPP_GEN_POSEIDON_SWAP) and of the generators a Merkle-opening circuit uses, and a CPU replay
of a level schedule (sipp_plonk_generate_witness_levels): the checker of the device witness of sipp_amd/merkle.py.

The swap row: s = W(swap); d_i = s (W(in+4+i) - W(in+i)) into W(delta+i); the state (in_i + d_i, in_(4+i) - d_i, in_8 .. in_11) goes through
tools/plonk_synth.poseidon_rows, whose S-box wires are re-based from its own offset to the gate's `sbox`; the outputs are checked against
the oracle's permutation (oracle/poseidon.c) on a sample of rows."""
import os
import sys

import numpy as np

from tests import _oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plonk_synth as ps  # noqa: E402

GEN_CONSTANT, GEN_PUBLIC_INPUT, GEN_BASE_SPLIT, GEN_RANDOM_ACCESS, GEN_POSEIDON, GEN_POSEIDON_SWAP = 3, 4, 2, 6, 8, 9


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


def run_generator(wires, consts, pih, g, rows):
    """one generator (kind, selector_index, row, p0 .. p4) on the given rows whose selector cell holds its gate index"""
    kind, si, gate, p = g[0], g[1], g[2], g[3:8]
    rows = np.asarray(rows, dtype=np.int64)
    rows = rows[consts[si, rows] == np.uint64(gate)]
    if not len(rows):
        return
    if kind == GEN_POSEIDON_SWAP:
        poseidon_rows(wires, rows, p[0], p[1], p[2], swap=p[3], delta=p[4])
    elif kind == GEN_POSEIDON:
        poseidon_rows(wires, rows, p[0], p[1], p[2])
    elif kind == GEN_CONSTANT:
        for l in range(p[0]):
            wires[l, rows] = consts[p[1] + l, rows]
    elif kind == GEN_PUBLIC_INPUT:
        for l in range(4):
            wires[l, rows] = np.uint64(int(pih[l]))
    elif kind == GEN_BASE_SPLIT:
        v, mask = wires[0, rows], np.uint64((1 << p[1]) - 1)
        for l in range(p[0]):
            wires[1 + l, rows] = (v >> np.uint64(p[1] * l)) & mask
    elif kind == GEN_RANDOM_ACCESS:
        bits, ln = p[2], 1 << p[2]
        for cp in range(p[0]):
            b = p[1] * cp
            idx = (wires[b, rows] & np.uint64(ln - 1)).astype(np.int64)
            wires[b + 1, rows] = wires[b + 2 + idx, rows]
            for l in range(bits):
                wires[b + 2 + ln + l, rows] = (idx >> l) & 1
    else:
        raise ValueError("no reading of generator kind %d" % kind)


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
