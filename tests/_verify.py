"""Both verifiers over one proof: the library's own (sipp_stark_verify: sipp_amd/csrc/verify.cpp, what a user of the library runs --
starky's verify_stark_proof / data.verify of reference src/verifier_circuit.rs:254) and the CPU oracle's (oracle/stark.c, the checker).
A proof counts as accepted only if BOTH accept; a refusal must come from both, at the same stage."""
import ctypes as C

import numpy as np

from tests import _oracle

u64p = C.POINTER(C.c_uint64)


def both_accept(proof, ocfg=None, cfg=None):
    import sipp_amd
    if cfg is None and ocfg is not None:
        cfg = sipp_amd.default_config()
        for name, _ in _oracle.OrcConfig._fields_:
            setattr(cfg, name, getattr(ocfg, name))
    a, b = sipp_amd.stark_verify(proof, cfg), _oracle.stark_verify(proof, ocfg)
    assert (a == 0) == (b == 0), "the verifiers disagree: library stage %d, oracle %d" % (a, b)
    return a == 0


def both_refuse(proof, ocfg=None, cfg=None):
    import sipp_amd
    if cfg is None and ocfg is not None:
        cfg = sipp_amd.default_config()
        for name, _ in _oracle.OrcConfig._fields_:
            setattr(cfg, name, getattr(ocfg, name))
    a, b = sipp_amd.stark_verify(proof, cfg), _oracle.stark_verify(proof, ocfg)
    assert a == -b, "the verifiers disagree: library stage %d, oracle %d" % (a, b)
    return a != 0


# ---- the generic proofs: oracle-side parameter structs in, the library's verdict (refusing stage, 0 = accepted) out ----
def lib_fri_params(ofp):
    import sipp_amd
    return sipp_amd.FriParams.from_buffer_copy(bytes(ofp))


def lib_plonk_verify(pf, cs_cap, p, ofp, circ, digest):
    import sipp_amd
    L = sipp_amd.lib()
    pf = np.ascontiguousarray(pf, dtype=np.uint64)
    cap = np.ascontiguousarray(cs_cap, dtype=np.uint64).reshape(-1)
    pp = sipp_amd.PlonkParams(p.num_routed_wires, p.max_degree, p.num_challenges)
    fp = lib_fri_params(ofp)
    cc = sipp_amd.PlonkCircuit.from_dict(circ)
    dg = np.asarray(digest, dtype=np.uint64)
    reason = C.c_int(0)
    rc = L.sipp_plonk_verify_gates(pf.ctypes.data_as(u64p), len(pf), cap.ctypes.data_as(u64p), C.byref(pp), C.byref(fp), C.byref(cc),
                                   dg.ctypes.data_as(u64p), C.byref(reason))
    assert rc in (0, -9), rc
    return reason.value


def lib_fri_verify(proof, caps, ncols, n_salt, batches, log_n, ofp, och):
    import sipp_amd
    L = sipp_amd.lib()
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    caps = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1) for c in caps]
    cp = (u64p * len(caps))(*[c.ctypes.data_as(u64p) for c in caps])
    nc = (C.c_uint32 * len(caps))(*ncols)
    ns = (C.c_uint32 * len(caps))(*n_salt)
    arr = (sipp_amd._lib.FriBatch * len(batches))()
    keep = []
    for i, (pt, ranges) in enumerate(batches):
        r = (sipp_amd._lib.PolyRange * len(ranges))(*[sipp_amd._lib.PolyRange(*x) for x in ranges])
        keep.append(r)
        arr[i].point[0], arr[i].point[1] = int(pt[0]), int(pt[1])
        arr[i].n_ranges = len(ranges)
        arr[i].ranges = r
    ch = sipp_amd.Challenger.from_buffer_copy(bytes(och))
    fp = lib_fri_params(ofp)
    reason = C.c_int(0)
    rc = L.sipp_fri_verify_openings(proof.ctypes.data_as(u64p), len(proof), cp, nc, ns, len(caps), arr, len(batches), log_n, C.byref(fp),
                                    C.byref(ch), C.byref(reason))
    assert rc in (0, -9), rc
    return reason.value, bytes(ch)


def py_plonk_replay(pf, circ, p, ofp, digest, pis):
    """the second reading (oracle/py/plonky2_generic.py) on a "SIPPPLK3" proof: the transcript from the proof's caps, the gate constraints
    at zeta from the OPENED constants and wires (evaluate_gate_constraints), the permutation terms, and per challenge whether the
    verifier's identity vanishing(zeta) = Z_H(zeta) quotient(zeta) holds"""
    from oracle.py import plonky2_generic as g2
    pf = [int(v) for v in pf]
    R, D, C = p.num_routed_wires, p.max_degree, p.num_challenges
    K, W, log_n = circ["num_constants"], circ["num_wires"], pf[1]
    pih = g2.hash_no_pad([int(x) for x in pis])
    cap_words = 4 << ofp.cap_height
    wcap, zcap, qcap = (pf[16 + k * cap_words:16 + (k + 1) * cap_words] for k in range(3))
    ch = g2.Challenger()
    ch.observe_many([int(x) for x in digest])
    ch.observe_many(pih)
    ch.observe_cap([wcap[4 * k:4 * k + 4] for k in range(1 << ofp.cap_height)])
    betas, gammas = ch.get_n(C), ch.get_n(C)
    ch.observe_cap([zcap[4 * k:4 * k + 4] for k in range(1 << ofp.cap_height)])
    alphas = ch.get_n(C)
    ch.observe_cap([qcap[4 * k:4 * k + 4] for k in range(1 << ofp.cap_height)])
    zeta = ch.get_ext()
    npd = _oracle.plonk_num_prods(p)
    op = pf[16 + 3 * cap_words + 8:]
    take = iter(range(0, 10 ** 9, 2))
    ext_at = lambda: (lambda k: g2.Ext(op[k], op[k + 1]))(next(take))
    c_o = [ext_at() for _ in range(K)]
    sg_o = [ext_at() for _ in range(R)]
    w_o = [ext_at() for _ in range(W)]
    zs_o = [ext_at() for _ in range(C)]
    pp_o = [ext_at() for _ in range(C * npd)]
    q_o = [ext_at() for _ in range(C * D)]
    zn_o = [ext_at() for _ in range(C)]
    terms = g2.evaluate_gate_constraints(circ["gates"], circ["programs"], circ["num_selectors"], w_o, c_o, pih)
    van = g2.eval_vanishing_poly_permutation(log_n, zeta, w_o[:R], sg_o, zs_o, zn_o, pp_o, betas, gammas, alphas, D, terms)
    zeta_n = zeta ** (1 << log_n)
    holds = []
    for c in range(C):
        acc = g2.ext(0)
        for d in reversed(range(D)):
            acc = acc * zeta_n + q_o[c * D + d]
        holds.append(van[c] == (zeta_n - g2.ext(1)) * acc)
    return holds
