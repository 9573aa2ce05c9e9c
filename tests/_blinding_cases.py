"""Zero-knowledge blinding (include/sipp_hip.h "ZERO KNOWLEDGE") read a second time, in exact Python integers, for
tests/test_blinding_reading.py (CPU) and tests/test_gpu_blinding.py:

  block()                     the one random function: a Poseidon permutation written out here from data/poseidon_goldilocks_rc.txt
  blocks()                    many blocks at once through the C oracle's permutation (the CPU test holds the two together at the edges)
  salt_columns / salt_natural the four salt columns of a stream in leaf order / in the natural order sipp_commit_batch_ex takes
  blind_fill                  SIPP_GEN_RANDOM on a wire table
  blinding_counts             plonky2's counting rule, restated
  BlindCircuit                the catalogue's circuit: an arithmetic row bound to a public input that a Poseidon chain hashes in circuit,
                              with or without two tagged lookup tables, with or without blinding rows
  read_proof5                 a verifier for "SIPPPLK5" composed from pieces the oracle exports: its challenger, the vanishing equation at
                              zeta over Python integers (permutation terms, the gate programs interpreted, the lookup terms of
                              tests/_lookup_tables_cases.py) and orc_fri_verify_openings with n_salt = {0, 4, 4, 4}

Nothing here imports the device library's kernels or its host verifier."""
import ctypes as C
import functools
import os

import numpy as np

from sipp_amd.circuit import _K, _W, P, PUBLIC_INPUT, CircuitBuilder, pi
from sipp_amd.merkle import declare_swap_gate
from tests import _lookup_cases as lc
from tests import _lookup_tables_cases as tc
from tests import _oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_UNSUPPORTED, E_VERIFY = -1, -7, -9
GEN_RANDOM = 18                        # include/sipp_hip.h SIPP_GEN_RANDOM
STREAM_ROWS, STREAM_WIRES, STREAM_ZS, STREAM_QUOTIENT = 0, 1, 2, 3
MAGIC5 = int.from_bytes(b"SIPPPLK5", "little")
MAGIC4 = int.from_bytes(b"SIPPPLK4", "little")

# ---- block(): one Poseidon permutation ------------------------------------------------------------------------------------------------
_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]


@functools.lru_cache(maxsize=None)
def _round_constants():
    vals = []
    for line in open(os.path.join(ROOT, "data", "poseidon_goldilocks_rc.txt")):
        vals += [int(t, 16) for t in line.split("#")[0].replace(",", " ").split()]
    assert len(vals) == 360
    return vals


def _permute(state):
    """4 full rounds, 22 partial rounds (the S-box on element 0 alone), 4 full rounds; out[r] = sum_c s[c] circ[(c - r) mod 12] + 8 s[0] [r = 0]"""
    rc, s = _round_constants(), [x % P for x in state]
    for rnd in range(30):
        s = [(x + rc[12 * rnd + i]) % P for i, x in enumerate(s)]
        if rnd < 4 or rnd >= 26:
            s = [pow(x, 7, P) for x in s]
        else:
            s[0] = pow(s[0], 7, P)
        s = [(sum(s[c] * _CIRC[(c - r) % 12] for c in range(12)) + (8 * s[0] if r == 0 else 0)) % P for r in range(12)]
    return s


def block(seed, counter, stream, index):
    """the first 8 words of hash_n_to_m_no_pad([seed0..3, counter, stream, index], 8): seven inputs fit the rate, so ONE permutation"""
    assert len(seed) == 4 and all(0 <= int(x) < P for x in seed)
    return _permute([int(x) for x in seed] + [int(counter), int(stream), int(index), 0, 0, 0, 0, 0])[:8]


@functools.lru_cache(maxsize=None)
def blocks(seed, counter, stream, count):
    """block(seed, counter, stream, i) for i < count as a [count][8] array, through the C oracle's permutation (25 k blocks in Python
    integers would take the tests' time; test_blinding_reading.py holds block() and that permutation together)"""
    L = orc.load()
    out = np.zeros((count, 8), dtype=np.uint64)
    st = np.zeros(12, dtype=np.uint64)
    for i in range(count):
        st[:] = 0
        st[:4] = np.array(seed, dtype=np.uint64)
        st[4], st[5], st[6] = counter, stream, i
        L.orc_poseidon_permute(st)
        out[i] = st[:8]
    return out


def salt_columns(seed, counter, stream, leaves):
    """[4][leaves] in LEAF order: leaf j takes words 4 (j & 1) .. 4 (j & 1) + 3 of block(.., stream, j >> 1)"""
    b = blocks(tuple(int(x) for x in seed), int(counter), int(stream), leaves // 2)
    out = np.zeros((4, leaves), dtype=np.uint64)
    for k in range(4):
        out[k, 0::2] = b[:, k]
        out[k, 1::2] = b[:, 4 + k]
    return out


def bitrev_index(log_m):
    idx = np.arange(1 << log_m)
    r = np.zeros_like(idx)
    for b in range(log_m):
        r |= ((idx >> b) & 1) << (log_m - 1 - b)
    return r


def salt_natural(seed, counter, stream, log_m):
    """the same columns in natural LDE order (what sipp_commit_batch_ex takes and bit-reverses): natural[i] = leaf[bitrev(i)]"""
    return np.ascontiguousarray(salt_columns(seed, counter, stream, 1 << log_m)[:, bitrev_index(log_m)])


def blind_fill(wires, consts, gens, seed, counter):
    """SIPP_GEN_RANDOM (kind, selector column, selector value, first wire, number of wires) on every row that holds it: wire w of row r
    takes word w & 7 of block(seed, counter, 0, r 2^9 + (w >> 3)) -> (the table afterwards, the mask of written cells)"""
    out, mask = wires.copy(), np.zeros(wires.shape, dtype=bool)
    for g in gens:
        if g[0] != GEN_RANDOM:
            continue
        sel, val, w0, cnt = g[1], g[2], g[3], g[4]
        for r in np.flatnonzero(consts[sel] == np.uint64(val)):
            cache = {}
            for w in range(w0, w0 + cnt):
                if w >> 3 not in cache:
                    cache[w >> 3] = block(seed, counter, STREAM_ROWS, (int(r) << 9) + (w >> 3))
                out[w][r], mask[w][r] = cache[w >> 3][w & 7], True
    return out, mask


def blinding_counts(num_queries, arity_bits, log_n):
    """(regular, z) with D = 2: fri_openings = num_queries (1 + D sum_rounds (2^arity_bits - 1) + final_poly_len)"""
    openings = num_queries * (1 + 2 * sum((1 << a) - 1 for a in arity_bits) + (1 << (log_n - sum(arity_bits))))
    return 2 + openings, 4 + openings


# ---- the catalogue's circuit ----------------------------------------------------------------------------------------------------------
GEN_ARITHMETIC = 1
ARITHMETIC, POSEIDON_SWAP = 4, 5
XOR4 = [(t >> 4) ^ (t & 15) for t in range(256)]
# whole proofs: log_n = 10, queries 2, three rounds of arity 4, final length 16 -> 72 regular rows and 74 pairs
PROOF_FRI = dict(rate_bits=3, cap_height=4, pow_bits=8, num_queries=2, arity_bits=2, final_poly_bits=4)
PROOF_LOG_N = 10
PROOF_DIGEST = (17, 0, P - 1, 1 << 32)
SEED = (0x0123456789ABCDEF, P - 1, 0, 0xFFFFFFFF)
COUNTERS = (0, (1 << 32) + 1)


def proof_fri(log_n, hiding=1):
    from sipp_amd.circuit import fri_params
    fp = fri_params(log_n, **PROOF_FRI)
    fp.hiding = hiding
    return fp


def arithmetic_into(pr, k0, k1):
    """one operation: w3 = c0 w0 w1 + c1 w2"""
    pr.constraint([(1, [(_W, 3)]), (-1, [(_K, k0), (_W, 0), (_W, 1)]), (-1, [(_K, k1), (_W, 2)])])


class BlindCircuit(CircuitBuilder):
    """a and b are witness inputs; x = 16 a + b comes from an arithmetic row.  Without lookups the public input is x; with them a and b
    are range-checked against a 16-entry table (tag 1) and the public input is y = xor4[x] from a function lookup (tag 0), as in
    tests/_lookup_tables_circuit.py.  A Poseidon chain hashes the public input in circuit.  blind: the gate Blind (a selector value of
    its own, no constraints) and the blinding rows of finish()."""
    n_public_args = 1

    def __init__(self, lookups=False, blind=True, min_log_n=PROOF_LOG_N, fri_of=proof_fri, num_wires=135, num_routed=80, **counts):
        names = ["Noop", "PublicInput", "Constant", "BaseSum", "Arithmetic", "PoseidonSwap"] + (["Table", "Looking"] if lookups else []) + ["Blind"]
        group = (0, 0, 0, 0, 0, 1) + ((2, 2) if lookups else ()) + (2,)
        CircuitBuilder.__init__(self, num_wires, num_routed, names, group, 2, 1)
        self.lookups, self.BLIND = lookups, len(names) - 1
        self.declare_basic(4)
        self.declare(ARITHMETIC, 3, (GEN_ARITHMETIC, 1, self.k0, self.k1), arithmetic_into, self.k0, self.k1)
        declare_swap_gate(self, POSEIDON_SWAP)
        if lookups:
            self.declare(6, 0)
            self.declare(7, 0)
            self.declare_lookup(6, 7, 2, 4, tables=True)
        self.declare(self.BLIND, 0)
        if blind:
            self.declare_blinding(self.BLIND, fri_of, **counts)
        self.pi_row = self.new_row(PUBLIC_INPUT)
        self.place(self.pi_row)
        zero, one = self.constant(0)[1], self.constant(1)[1]
        a, b = self.witness_input(), self.witness_input()
        if lookups:
            self.xor4 = self.function_table(XOR4)
            self.range16 = self.table([(v, 0) for v in range(16)])
            self.range_check(a, self.range16)
            self.range_check(b, self.range16)
        self.x_row = self.new_row(ARITHMETIC, 16, 1)
        self.place(self.x_row, [(0, a), (1, one), (2, b)])
        out = (3, self.x_row)
        if lookups:
            out, = self.function_lookup(self.xor4, [out])
        self.tie(pi(0), out)
        self.hash_public_inputs(POSEIDON_SWAP, zero)
        self.finish(min_log_n)

    def value(self, a, b):
        return XOR4[16 * a + b] if self.lookups else 16 * a + b

    def public_inputs(self, y):
        return [int(y) % P]

    def input_cells(self, y, a, b):
        cells, values = [], []
        for cyc, v in zip(self.pi_cycle + self.in_cycle, (y, a, b)):
            cells += cyc
            values += [int(v) % P] * len(cyc)
        return np.array(cells, dtype=np.uint64), np.array(values, dtype=np.uint64)

    def words_map(self):
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


@functools.lru_cache(maxsize=None)
def circuit(lookups, blind=True):
    return BlindCircuit(lookups=lookups, blind=blind)


# ---- the composed verifier ------------------------------------------------------------------------------------------------------------
class _Transcript:
    """the oracle's challenger (orc_chal_*), whose state orc_fri_verify_openings takes over"""

    def __init__(self):
        self.L = orc.load()
        self.ch = orc.challenger()
        self.L.orc_chal_get.restype = C.c_uint64
        self.L.orc_chal_get.argtypes = [C.POINTER(orc.OrcChallenger)]

    def observe(self, words):
        for w in words:
            self.L.orc_chal_observe(C.byref(self.ch), int(w))

    def get(self):
        return int(self.L.orc_chal_get(C.byref(self.ch)))

    def copy(self):
        t = _Transcript.__new__(_Transcript)
        t.L, t.ch = self.L, orc.OrcChallenger.from_buffer_copy(self.ch)
        return t


def _gate_terms_at_zeta(circ, cv, wv, pih):
    """term j = sum_g filter_g(selector at zeta) constraint_(g, j), the programs interpreted over the extension"""
    ngc = max(g[5] for g in circ["gates"])
    out = [(0, 0)] * ngc
    prog = [int(x) for x in circ["programs"]]
    for sel_col, row, lo, hi, off, cnt in circ["gates"]:
        f, sel = (1, 0), cv[sel_col]
        for i in range(lo, hi):
            if i != row:
                f = lc.e2_mul(f, lc.e2_sub((i, 0), sel))
        if circ["num_selectors"] > 1:
            f = lc.e2_mul(f, lc.e2_sub((0xFFFFFFFF, 0), sel))
        at = off
        for j in range(cnt):
            nm, at, total = prog[at], at + 1, (0, 0)
            for _ in range(nm):
                t, nf, at = (prog[at] % P, 0), prog[at + 1], at + 2
                for _ in range(nf):
                    kind, idx, at = prog[at], prog[at + 1], at + 2
                    t = lc.e2_mul(t, wv[idx] if kind == 0 else cv[idx] if kind == 1 else (pih[idx], 0))
                total = lc.e2_add(total, t)
            out[j] = lc.e2_add(out[j], lc.e2_mul(f, total))
    return out


def parse5(proof, circ, fp, D, C, n_pi):
    """the sections of a flat "SIPPPLK5" proof -> a dict, or the name of what fails: "header" """
    pf = [int(v) for v in proof]
    desc = tuple(int(x) for x in circ.get("lookup", (0,) * 8))
    W, K, R = circ["num_wires"], circ["num_constants"], circ["num_routed"]
    ngc = max(g[5] for g in circ["gates"])
    n_cap, hw = 1 << fp.cap_height, 24
    if fp.hiding != 1 or len(pf) < hw + 12 * n_cap + 8 + n_pi or pf[0] != MAGIC5 or pf[2:5] != [R, D, C] or pf[5] != len(pf):
        return "header"
    if pf[6:12] != [W, K, circ["num_selectors"], len(circ["gates"]), ngc, n_pi] or pf[12:16] != [1, 0, 0, 0] or pf[16:24] != list(desc):
        return "header"
    if any(v >= P for v in pf[hw:]):
        return "header"
    m = -(-R // D)
    J = len(tc.group_slots(desc, D)) if any(desc) else 0
    nz, nlk = C * m, C * J
    at = hw + 12 * n_cap
    n0 = K + R + W + nz + nlk + C * D
    n_open = n0 + C + (C if J else 0)
    if len(pf) < at + 8 + 2 * n_open + n_pi:
        return "header"
    return {"pf": pf, "desc": desc, "log_n": pf[1], "caps": [pf[hw + 4 * n_cap * o: hw + 4 * n_cap * (o + 1)] for o in range(3)],
            "section": pf[at:len(pf) - n_pi], "pis": pf[len(pf) - n_pi:], "n0": n0, "n_open": n_open, "m": m, "J": J, "nz": nz, "nlk": nlk,
            "opened": [(pf[at + 8 + 2 * k], pf[at + 8 + 2 * k + 1]) for k in range(n_open)], "section_at": at}


def transcript_to_zeta(s, digest, C):
    """the challenges up to zeta -> (transcript, betas, gammas, etas, thetas, alphas, zeta, pih)"""
    pih = [int(x) for x in orc.hash_no_pad(s["pis"])] if s["pis"] else [0, 0, 0, 0]
    ch = _Transcript()
    ch.observe(list(digest) + pih + s["caps"][0])
    betas, gammas = [ch.get() for _ in range(C)], [ch.get() for _ in range(C)]
    etas, thetas = ([ch.get() for _ in range(C)], [ch.get() for _ in range(C)]) if s["J"] else ([], [])
    ch.observe(s["caps"][1])
    alphas = [ch.get() for _ in range(C)]
    ch.observe(s["caps"][2])
    zeta = (ch.get(), ch.get())
    return ch, betas, gammas, etas, thetas, alphas, zeta, pih


def read_proof5(proof, circ, cs_cap, digest, fp, D, C, n_pi):
    """-> None for an accepted proof, else "header", "vanishing" or ("fri", the oracle's stage)"""
    s = parse5(proof, circ, fp, D, C, n_pi)
    if isinstance(s, str):
        return s
    W, K, R = circ["num_wires"], circ["num_constants"], circ["num_routed"]
    desc, log_n, m, J, nz, nlk, n0, v = s["desc"], s["log_n"], s["m"], s["J"], s["nz"], s["nlk"], s["n0"], s["opened"]
    ch, betas, gammas, etas, thetas, alphas, zeta, pih = transcript_to_zeta(s, digest, C)
    cv, sg, wv = v[:K], v[K:K + R], v[K + R:K + R + W]
    zs = v[K + R + W:]
    npp = m - 1
    pps, ss, us, qs = zs[C:nz], zs[nz:nz + C], zs[nz + C:nz + nlk], zs[nz + nlk:nz + nlk + C * D]
    zs_next, ss_next = v[n0:n0 + C], v[n0 + C:]
    n = 1 << log_n
    zeta_n = lc.e2_pow(zeta, n)
    zh = lc.e2_sub(zeta_n, (1, 0))
    l0 = lc.e2_mul(zh, lc.e2_inv(lc.e2_scale(lc.e2_sub(zeta, (1, 0)), n)))
    terms = [lc.e2_mul(l0, lc.e2_sub(zs[c], (1, 0))) for c in range(C)]
    for c in range(C):
        for q in range(m):
            num = den = (1, 0)
            for j in range(q * D, min((q + 1) * D, R)):
                g = (gammas[c], 0)
                num = lc.e2_mul(num, lc.e2_add(lc.e2_add(wv[j], lc.e2_scale(zeta, betas[c] * pow(7, j, P) % P)), g))
                den = lc.e2_mul(den, lc.e2_add(lc.e2_add(wv[j], lc.e2_scale(sg[j], betas[c])), g))
            prev = zs[c] if q == 0 else pps[c * npp + q - 1]
            nxt = zs_next[c] if q == npp else pps[c * npp + q]
            terms.append(lc.e2_sub(lc.e2_mul(prev, num), lc.e2_mul(nxt, den)))
    terms += _gate_terms_at_zeta(circ, cv, wv, pih)
    if J:
        terms += tc.lookup_terms_at_zeta(desc, D, C, cv, wv, ss, us, ss_next, l0, etas, thetas)
    for c in range(C):
        van = (0, 0)
        for t in reversed(terms):
            van = lc.e2_add(lc.e2_scale(van, alphas[c]), t)
        acc = (0, 0)
        for d in reversed(range(D)):
            acc = lc.e2_add(lc.e2_mul(acc, zeta_n), qs[c * D + d])
        if van != lc.e2_mul(zh, acc):
            return "vanishing"
    rc = orc.fri_verify_openings(np.array(s["section"], dtype=np.uint64), fri_caps(s, cs_cap), [K + R, W, nz + nlk, C * D], [0, 4, 4, 4],
                                 fri_batches(s, zeta, K, R, W, C, D), log_n, orc_fri(fp), ch.ch)
    return None if rc == 0 else ("fri", rc)


def fri_caps(s, cs_cap):
    return [np.asarray(cs_cap, dtype=np.uint64).reshape(-1)] + [np.array(c, dtype=np.uint64) for c in s["caps"]]


def fri_batches(s, zeta, K, R, W, C, D):
    nz, nzl = s["nz"], s["nz"] + s["nlk"]
    w = pow(lc.ROOT32, 1 << (32 - s["log_n"]), P)
    return [(zeta, [(0, 0, K + R), (1, 0, W), (2, 0, nzl), (3, 0, C * D)]),
            (lc.e2_scale(zeta, w), [(2, 0, C)] + ([(2, nz, nz + C)] if s["J"] else []))]


def orc_fri(fp):
    return orc.fri_params(rate_bits=fp.rate_bits, cap_height=fp.cap_height, pow_bits=fp.pow_bits, num_queries=fp.num_queries,
                          pow_rule=fp.pow_rule, hiding=fp.hiding, arities=[fp.arity_bits[r] for r in range(fp.n_rounds)])


def query_rounds(proof, circ, digest, fp, D, C, n_pi):
    """[(leaf index x, {oracle: its leaf words, salt last})] of every query round: the transcript run on through the opening section
    (opened values, alpha, the rounds' caps and betas, the final polynomial, the proof-of-work witness under rule 0, the indices)"""
    s = parse5(proof, circ, fp, D, C, n_pi)
    assert not isinstance(s, str) and fp.pow_rule == 0
    W, K, R = circ["num_wires"], circ["num_constants"], circ["num_routed"]
    ch = transcript_to_zeta(s, digest, C)[0]
    sec, log_n = s["section"], s["log_n"]
    at = 8 + 2 * s["n_open"]
    ch.observe(sec[8:at])
    ch.get(), ch.get()                                  # alpha
    n_cap, arity = 1 << fp.cap_height, [fp.arity_bits[r] for r in range(fp.n_rounds)]
    for _ in arity:
        ch.observe(sec[at:at + 4 * n_cap])
        at += 4 * n_cap
        ch.get(), ch.get()                              # the round's fold challenge
    flen = (1 << log_n) >> sum(arity)
    ch.observe(sec[at:at + 2 * flen])
    at += 2 * flen
    ch.observe([sec[at]])
    at += 1
    ch.get()                                            # the proof-of-work response
    log_m = log_n + fp.rate_bits
    xs = [ch.get() % (1 << log_m) for _ in range(fp.num_queries)]
    ncols, salt, ns0 = [K + R, W, s["nz"] + s["nlk"], C * D], [0, 4, 4, 4], log_m - fp.cap_height
    qwords, lt = sum(ncols) + sum(salt) + 4 * 4 * ns0, log_m
    for a in arity:
        lt -= a
        qwords += (2 << a) + 4 * max(lt - fp.cap_height, 0)
    out = []
    for qi, x in enumerate(xs):
        q, leaves, where = at + qi * qwords, {}, {}
        for o in range(4):
            leaves[o], where[o] = sec[q:q + ncols[o] + salt[o]], s["section_at"] + q
            q += ncols[o] + salt[o] + 4 * ns0
        out.append((x, leaves, where))
    return out
