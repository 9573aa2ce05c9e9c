"""An independent reading, in Python integers, of what plonky2's verifier computes before the FRI check (plonk/verifier.rs with
vanishing_poly.rs's eval_vanishing_poly, recalled) from a flat "SIPPPLK3" proof: the challenges, zeta^n, Z_H, L_0, every term, both
sides of the closing equality per challenge and the sponge state the FRI verifier takes over.  Imports nothing from
sipp_amd/plonk_vanishing.py; the permutation is the CPU oracle's."""
import numpy as np

from tests import _oracle

P = _oracle.P
W = 7                                                           # F[X] / (X^2 - 7)
HEADER, FRI_HEADER = 16, 8


def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_inv(a):
    n = pow((a[0] * a[0] - W * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def base(x):
    return (x % P, 0)


class Sponge:
    """the duplex challenger: eight inputs, or a draw with inputs pending or nothing left, permute; draws pop from the rate's end"""

    def __init__(self):
        self.state, self.inputs, self.outputs = [0] * 12, [], []

    def _permute(self):
        self.state[:len(self.inputs)] = self.inputs
        self.state = [int(v) for v in _oracle.permute(np.array(self.state, dtype=np.uint64))]
        self.inputs, self.outputs = [], self.state[:8]

    def observe(self, words):
        for v in words:
            self.outputs = []
            self.inputs.append(int(v))
            if len(self.inputs) == 8:
                self._permute()

    def draw(self):
        if self.inputs or not self.outputs:
            self._permute()
        return self.outputs.pop()


def split(proof, circ, params, cap_height, n_pi):
    """the flat proof -> dict(caps, constants, sigmas, wires, zs, pps, quotient, zs_next, public_inputs), ext values as pairs"""
    R, D, C = params
    pf = [int(v) for v in proof]
    n_cap, m = 1 << cap_height, -(-R // D)
    caps = [pf[HEADER + 4 * n_cap * o:HEADER + 4 * n_cap * (o + 1)] for o in range(3)]
    at = [HEADER + 12 * n_cap + FRI_HEADER]

    def take(k):
        out = [(pf[at[0] + 2 * i], pf[at[0] + 2 * i + 1]) for i in range(k)]
        at[0] += 2 * k
        return out
    out = {"caps": caps, "constants": take(circ["num_constants"]), "sigmas": take(R), "wires": take(circ["num_wires"]), "zs": take(C),
           "pps": take(C * (m - 1)), "quotient": take(C * D), "zs_next": take(C), "public_inputs": pf[len(pf) - n_pi:]}
    out["opened_at"], out["opened_end"] = HEADER + 12 * n_cap + FRI_HEADER, at[0]
    return out


def read(proof, digest, log_n, circ, params, cap_height, n_pi):
    """-> dict(pih, betas, gammas, alphas, zeta, gzeta, state, zeta_n, zh, l0, terms, sides = per challenge (vanishing, Z_H quotient))"""
    R, D, C = params
    s = split(proof, circ, params, cap_height, n_pi)
    pih = [int(v) for v in _oracle.hash_no_pad(np.array(s["public_inputs"], dtype=np.uint64))]
    sp = Sponge()
    sp.observe(list(digest) + pih + s["caps"][0])
    betas = [sp.draw() for _ in range(C)]
    gammas = [sp.draw() for _ in range(C)]
    sp.observe(s["caps"][1])
    alphas = [sp.draw() for _ in range(C)]
    sp.observe(s["caps"][2])
    zeta = (sp.draw(), sp.draw())
    n = 1 << log_n
    zeta_n = zeta
    for _ in range(log_n):
        zeta_n = e_mul(zeta_n, zeta_n)
    zh = e_sub(zeta_n, base(1))
    l0 = e_mul(zh, e_inv(e_mul(base(n), e_sub(zeta, base(1)))))
    m = -(-R // D)
    terms = [e_mul(l0, e_sub(z, base(1))) for z in s["zs"]]
    for c in range(C):
        for q in range(m):
            num = s["zs"][c] if q == 0 else s["pps"][c * (m - 1) + q - 1]
            den = s["zs_next"][c] if q == m - 1 else s["pps"][c * (m - 1) + q]
            for j in range(q * D, min((q + 1) * D, R)):
                shifted = e_mul(base(betas[c] * pow(7, j, P)), zeta)
                num = e_mul(num, e_add(e_add(s["wires"][j], shifted), base(gammas[c])))
                den = e_mul(den, e_add(e_add(s["wires"][j], e_mul(base(betas[c]), s["sigmas"][j])), base(gammas[c])))
            terms.append(e_sub(num, den))
    terms += gate_terms(circ, s["wires"], s["constants"], pih)
    sides = []
    for c in range(C):
        van = (0, 0)
        for t in reversed(terms):
            van = e_add(e_mul(van, base(alphas[c])), t)
        acc = (0, 0)
        for d in reversed(range(D)):
            acc = e_add(e_mul(acc, zeta_n), s["quotient"][c * D + d])
        sides.append((van, e_mul(zh, acc)))
    g = pow(1753635133440165772, 1 << (32 - log_n), P)
    return {"pih": pih, "betas": betas, "gammas": gammas, "alphas": alphas, "zeta": zeta, "gzeta": (zeta[0] * g % P, zeta[1] * g % P),
            "state": list(sp.state), "zeta_n": zeta_n, "zh": zh, "l0": l0, "terms": terms, "sides": sides, "split": s}


def gate_terms(circ, wires, constants, pih):
    """term j = the sum over the gates of filter times constraint j, from the program words"""
    prog = [int(x) for x in circ["programs"]]
    out = [(0, 0)] * max(g[5] for g in circ["gates"])
    for sel, row, lo, hi, w, ncons in circ["gates"]:
        f = base(1)
        for i in range(lo, hi):
            if i != row:
                f = e_mul(f, e_sub(base(i), constants[sel]))
        if circ["num_selectors"] > 1:
            f = e_mul(f, e_sub(base(0xFFFFFFFF), constants[sel]))
        for j in range(ncons):
            nm, w = prog[w], w + 1
            total = (0, 0)
            for _ in range(nm):
                t, nf = base(prog[w]), prog[w + 1]
                w += 2
                for _ in range(nf):
                    kind, idx = prog[w], prog[w + 1]
                    w += 2
                    t = e_mul(t, wires[idx] if kind == 0 else constants[idx] if kind == 1 else base(pih[idx]))
                total = e_add(total, t)
            out[j] = e_add(out[j], e_mul(f, total))
    return out


def distinct_monomials(circ, gate):
    """how many different factor multisets the gate's program names"""
    prog, (_, _, _, _, w, ncons) = [int(x) for x in circ["programs"]], circ["gates"][gate]
    seen = set()
    for _ in range(ncons):
        nm, w = prog[w], w + 1
        for _ in range(nm):
            nf = prog[w + 1]
            seen.add(tuple(sorted((prog[w + 2 + 2 * f], prog[w + 3 + 2 * f]) for f in range(nf))))
            w += 2 + 2 * nf
    return len(seen)
