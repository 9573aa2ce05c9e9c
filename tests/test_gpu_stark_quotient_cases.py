"""The STARK prover's Z and quotient kernels on the crafted cells of tests/_stark_quotient_cases.py, against three readings.

sipp_k_z_columns (z_phase_a<4> / <8>, z_phase_b, z_phase_c) and sipp_k_quotient (quotient_prog_kernel<POLY> / <!POLY>,
quotient_rest_kernel<SPLIT> / <!SPLIT>, quotient_finish_kernel, alpha_pow3_kernel) are entered through tests/probe/stark_probe.hip on the
caller's cells and challenges, not through a whole proof, and compared WORD FOR WORD with

  orc_eval_base / Z_H       oracle/air.c through orc_quotient_points: at every point for log_n <= 13, at a fixed sample of 4096 points of
                            the g2_u16 table at log_n = 15 (built on the device from the catalogue's formula)
  eval_constraints / Z_H    oracle/py/stark_verify.py in Python integers, at the sampled points of the CPU test
  z_reference               Z[0] = 1, Z[r + 1] = Z[r] num[r] inv0(den[r]) cell by cell in Python integers (n <= 2^14); at 2^20 the defining
                            relation Z[r + 1] den[r] == Z[r] num[r] on every row

No tolerances.  What the cases reach (routes, the RestAcc fold, the sliced gadget, the q * p carry, the POLY coefficient paths, the chunk
loops of z_phase_b) is asserted without a device in tests/test_oracle_stark_quotient_cases.py.

Checked by hand against two mutations of prover.hip (neither committed):
  `(l < al ? 1u : 0u)` -> `0u` in quotient_prog_kernel     all fourteen `carry` cases fail, and the lattice table at log_n = 15
  `terms >= 960` -> `terms >= 100000` in RestAcc          the `fold` table at log_n = 15 fails (alpha = (p - 1, p - 1), pin - ptab =
      Z - 1 = p - 1: sum 4 of RestAcc F passes 2^64 -- sq.rest_f_peak); the all-(p - 1) and lattice tables there do not: with every cell
      p - 1, pin - ptab = 0 and the weights of Z - 1 are powers of a random alpha, whose limbs average half their range
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _oracle
from tests import _stark_quotient_cases as sq

pytestmark = pytest.mark.gpu

P = sq.P
PROBE_DIR = os.path.join(_oracle.ROOT, "tests", "probe")
SENTINEL = 0x5A5A5A5A5A5A5A5A
SIPP_E_UNSUPPORTED = -7


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


class Probe:
    """tests/probe/libstark_probe.so through ctypes, and the ctx whose stream and arena the stage drivers use"""

    def __init__(self):
        import torch  # noqa: F401  (first: the library binds to torch's HIP runtime)
        import sipp_amd
        self.ctx = sipp_amd.Ctx(workspace_bytes=1 << 30)
        subprocess.check_call(["make", "-C", PROBE_DIR, "-s"])
        L = C.CDLL(os.path.join(PROBE_DIR, "libstark_probe.so"))
        vp, u64x2 = C.c_void_p, C.c_uint64 * 2
        L.probe_air_info.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_int)]
        L.probe_quotient.argtypes = [vp, C.c_int, C.c_uint32, vp, vp, C.c_size_t, vp, u64x2, u64x2, u64x2, vp]
        L.probe_z_columns.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, u64x2, u64x2, vp]
        L.probe_rest_chunks.argtypes = [C.c_uint32, C.c_int]
        L.probe_rest_chunks.restype = C.c_uint32
        self.L, self.pair = L, lambda v: u64x2(int(v[0]), int(v[1]))

    def air_info(self, i):
        name, info = C.create_string_buffer(32), (C.c_int * 9)()
        assert self.L.probe_air_info(i, name, info) == 0
        return name.value.decode(), list(info)

    def quotient(self, case, lde, zlde, aux, alpha=None):
        """-> (status, out [2][m] as numpy); out is filled with SENTINEL first"""
        import torch
        m = 2 << case.log_n
        assert lde.shape[1] == zlde.shape[1] == aux.shape[1] == m
        out = torch.full((2, m), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = self.L.probe_quotient(self.ctx.h, case.ai, case.log_n, lde.data_ptr(), zlde.data_ptr(), m, aux.data_ptr(),
                                   self.pair(alpha or case.alpha), self.pair(case.beta), self.pair(case.gamma), out.data_ptr())
        return rc, host(out)

    def z_columns(self, case, trace):
        import torch
        zv = torch.full((2 * case.nc, 1 << case.log_n), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = self.L.probe_z_columns(self.ctx.h, case.n_main, case.cbase, case.nc, trace.data_ptr(), case.log_n, self.pair(case.beta),
                                    self.pair(case.gamma), zv.data_ptr())
        assert rc == 0, "probe_z_columns: %d" % rc
        return host(zv)


@pytest.fixture(scope="module")
def probe():
    p = Probe()
    yield p
    p.ctx.close()


def test_probe_sees_the_catalogues_airs_and_route_rule(probe):
    assert probe.L.probe_air_count() == len(sq.AIRS)
    for i, a in enumerate(sq.AIRS):
        keys = ("kind", "table_bits", "n_main", "checked_base", "n_checked", "n_aux", "n_gadgets", "log_rows", "hardened")
        assert probe.air_info(i) == (a["name"], [a[k] for k in keys])
    for log_n in range(10, 17):
        for nc in (1, 31, 32, 63, 64, 65, 126, 189, 378, 511, 512, 513, 1512):
            assert probe.L.probe_rest_chunks(log_n, nc) == sq.rest_chunks(log_n, nc), (log_n, nc)


def first_difference(got, want):
    ch, j = np.argwhere(got != want)[0]
    return "challenge %d, leaf position %d: device %#x, reference %#x (%d of %d words differ)" % (
        ch, j, int(got[ch, j]), int(want[ch, j]), int((got != want).sum()), got.size)


QCASES = sq.quotient_cases()


@pytest.mark.parametrize("case", QCASES, ids=[c.name for c in QCASES])
def test_quotient_on_crafted_cells(probe, case):
    lde, zlde, aux = sq.tables(case)
    d = [dev(t) for t in (lde, zlde, aux)]
    alpha = case.alpha
    if sq.refused(case):
        # alpha = 0 in either component: refused before any launch, the output untouched, and the ctx serves the next call
        rc, out = probe.quotient(case, *d)
        assert rc == SIPP_E_UNSUPPORTED and (out == SENTINEL).all()
        alpha = tuple(a or sq.LATTICE[2] for a in alpha)
        case = case._replace(alpha=alpha)
    rc, out = probe.quotient(case, *d, alpha=alpha)
    assert rc == 0, "probe_quotient: %d" % rc
    pos = np.arange(2 << case.log_n, dtype=np.uint32)
    want = _oracle.quotient_points(case.ai, case.log_n, lde, zlde, aux, alpha, case.beta, case.gamma, pos)
    assert (out == want).all(), "%s: the device leaves orc_eval_base / Z_H at %s" % (case.name, first_difference(out, want))
    # the Python reading at the CPU test's sampled points
    for j in sq.sample_positions(case.log_n):
        py = sq.python_quotient(case, lambda c, p: int(lde[c, p]), lambda c, p: int(zlde[c, p]), lambda c, p: int(aux[c, p]), int(j))
        assert [int(out[0, j]), int(out[1, j])] == py, "%s: the device leaves eval_constraints / Z_H at leaf position %d" % (case.name, j)


BIG = sq.big_cases()


@pytest.mark.parametrize("case", BIG, ids=[c.name for c in BIG])
def test_quotient_unsplit_walk_of_378_columns_at_log_n_15(probe, case):
    """g2_u16 at log_n = 15: quotient_rest_kernel<false> walks 378 checked columns and RestAcc folds -- in the `fold` case it must, or a
    sum wraps.  About 1.1 GB of cells, built on the device from the catalogue's formula; the references read a gather of the sampled
    points and their next rows, built on the host from the same formula."""
    import torch
    a = sq.AIRS[case.ai]
    log_m, m = case.log_n + 1, 2 << case.log_n
    nm, nc = a["n_main"], a["n_checked"]
    W, nz, na = nm + 2 * nc, 2 * nc, a["n_aux"]
    if case.style == "pm1":
        tabs = [torch.full((ncols, m), P - 1 - (1 << 64), dtype=torch.int64, device="cuda") for ncols in (W, nz, na)]
    else:
        lat, nat, tabs = dev(sq.LAT_U64), dev(sq.bitrev(log_m).astype(np.int64)), []
        for cls, ncols in ((sq.lde_classes(a), W), (np.full(nz, sq.ZCOL), nz), (np.full(na, sq.AUX), na)):
            idx = sq.lattice_index(dev(cls.astype(np.int64))[:, None], torch.arange(ncols, device="cuda")[:, None], nat[None, :])
            tabs.append(lat[idx])
            del idx
        if case.style == "fold":        # sq.class_tables: permuted inputs 0, permuted tables 1, Z 0
            tabs[0][nm:nm + nc], tabs[0][nm + nc:] = 0, 1
            tabs[1].zero_()
    rc, out = probe.quotient(case, *tabs)
    assert rc == 0
    pos = sq.big_sample(case.log_n)
    need, slot, want_cells = sq.big_gather(case, pos)
    gather = dev(need)
    lde, zlde, aux = (np.ascontiguousarray(host(t[:, gather])) for t in tabs)
    for got_cells, w in zip((lde, zlde, aux), want_cells):      # the device-built table IS the catalogue's formula
        assert (got_cells == w).all()
    want = _oracle.quotient_points(case.ai, case.log_n, lde, zlde, aux, case.alpha, case.beta, case.gamma, pos, slot)
    got = out[:, pos]
    assert (got == want).all(), "%s: the device leaves orc_eval_base / Z_H at %s (index into the sample)" % (case.name, first_difference(got, want))
    few = pos[[0, 1, 63, 64, 2000, 2001, 4094, 4095]]
    assert (out[:, few] == sq.check_two_readings(case, lde, zlde, aux, few, slot)).all()


# ---------------------------------------------------------------------------------------------------- Z
SMALL_Z = [c for c in sq.z_cases() if c.log_n <= 14]


@pytest.mark.parametrize("case", SMALL_Z, ids=[c.name for c in SMALL_Z])
def test_z_columns_on_crafted_cells(probe, case):
    trace = sq.z_trace(case)
    want = sq.z_reference(case, trace)
    got = probe.z_columns(case, dev(trace))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), "%s: Z column(s) %s leave the cell-by-cell rule; column %d: device %s..., reference %s..." % (
        case.name, bad[:8], bad[0], [hex(int(x)) for x in got[bad[0], :4]], [hex(int(x)) for x in want[bad[0], :4]])


def test_z_columns_relation_at_two_to_the_twenty(probe):
    """512 blocks of 256 x 8 rows: the prefix and the suffix loop of z_phase_b both cross a chunk of 256 block totals"""
    for case in (c for c in sq.z_cases() if c.log_n == 20):
        assert sq.z_blocks(case.log_n) == 512
        trace = sq.z_trace(case)
        got = probe.z_columns(case, dev(trace))
        assert sq.z_relation_holds(case, trace, got), case.name
        assert (got == _oracle.z_columns(trace, case.n_main, case.cbase, case.nc, case.beta, case.gamma)).all(), case.name


# ---------------------------------------------------------------------------------------------------- the probe's calling convention
def test_probe_convention_is_the_provers_on_an_honest_trace(probe):
    """g1_u8 at log_n = 10 (two records of the n = 4 SIPP fixture): the probe's Z and quotient on the oracle's honest trace, its LDE and
    the challenges of the oracle's proof transcript are the oracle's Z and quotient -- the very ones its proof commits to (their caps)"""
    L = _oracle.load()
    ios = np.load(os.path.join(_oracle.ROOT, "tests", "golden", "sipp_n4_ios.npz"))["g1"][:2]
    t = _oracle.Trace(0, ios)
    a = sq.AIRS[sq.G1_U8]
    nm, cb, nc, na, log_n = a["n_main"], a["checked_base"], a["n_checked"], a["n_aux"], 10
    n, m, W = 1 << log_n, 2 << log_n, nm + 2 * nc
    assert (t.log_n, t.width, t.air.name.decode()) == (log_n, W, "g1_u8")
    trace = t.array().copy()
    proof = _oracle.stark_prove_trace(t)
    cfg = _oracle.default_config()
    ncap = 1 << cfg.cap_height
    caps = [np.ascontiguousarray(proof[16 + 4 * ncap * k: 16 + 4 * ncap * (k + 1)]) for k in range(3)]
    # the transcript up to alpha: statement, root of the records, trace cap -> (beta, gamma) x 2, Z cap -> alpha x 2
    ppi = a["pi_per_io"]
    pis = np.ctypeslib.as_array(t.p.contents.pis, shape=(t.num_io * ppi,)).copy()
    root = np.zeros(4, dtype=np.uint64)
    L.orc_pi_root.argtypes = [_oracle.u32p, C.c_size_t, C.c_int, _oracle.u64p]
    L.orc_pi_root(pis, t.num_io, ppi, root)
    st = [0, log_n, t.num_io, W, 2 * nc, 4, cfg.rate_bits, cfg.cap_height, cfg.pow_bits, cfg.arity_bits, cfg.final_poly_bits, cfg.num_queries,
          cfg.num_challenges, cfg.pow_rule, ppi, cfg.lookup_rule]
    ch = _oracle.challenger(st + [int(x) for x in root])
    chp = C.POINTER(_oracle.OrcChallenger)
    L.orc_chal_observe_cap.argtypes = [chp, _oracle.u64p, C.c_size_t]
    L.orc_chal_get.argtypes, L.orc_chal_get.restype = [chp], C.c_uint64
    L.orc_chal_observe_cap(C.byref(ch), caps[0], ncap)
    bg = [L.orc_chal_get(C.byref(ch)) for _ in range(4)]
    beta, gamma = (bg[0], bg[2]), (bg[1], bg[3])
    # Z
    zv = _oracle.z_columns(trace, nm, cb, nc, beta, gamma)
    zb = _oracle.Batch(zv, log_n)
    assert (zb.cap.reshape(-1) == caps[1]).all(), "the transcript's challenges do not give the proof's Z"
    zcase = sq.ZCase("honest", log_n, nm, cb, nc, "honest", beta, gamma, 0, ())
    assert (probe.z_columns(zcase, dev(trace)) == zv).all()
    # quotient
    L.orc_chal_observe_cap(C.byref(ch), caps[1], ncap)
    alpha = (L.orc_chal_get(C.byref(ch)), L.orc_chal_get(C.byref(ch)))
    lde = np.ascontiguousarray(_oracle.Batch(trace, log_n).leaves.T)
    zlde = np.ascontiguousarray(zb.leaves.T)
    rev = sq.bitrev(log_n + 1)
    L.orc_aux_coeffs.argtypes = [C.c_void_p, _oracle.u32p, C.c_size_t, C.c_uint, C.c_int, _oracle.u64p]
    aux = np.zeros((na, m), dtype=np.uint64)
    for ai in range(na):
        co, nat = np.zeros(n, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        L.orc_aux_coeffs(C.cast(t.p.contents.air, C.c_void_p), pis, t.num_io, log_n, ai, co)
        L.orc_coset_lde(co, log_n, 1, sq.GEN, nat)
        aux[ai] = nat[rev]
    qcase = sq.QCase("honest", sq.G1_U8, log_n, "honest", alpha, beta, gamma, 0)
    rc, out = probe.quotient(qcase, dev(lde), dev(zlde), dev(aux))
    assert rc == 0
    want = _oracle.quotient_points(sq.G1_U8, log_n, lde, zlde, aux, alpha, beta, gamma, np.arange(m, dtype=np.uint32))
    assert (out == want).all(), first_difference(out, want)
    # ... and it is the quotient the proof commits to: coset inverse transform, four chunks of N coefficients, their cap
    chunks = np.zeros((4, n), dtype=np.uint64)
    shift_inv = pow(sq.GEN, -1, P)
    for i in range(2):
        co = np.ascontiguousarray(out[i][rev])
        L.orc_ifft(co, log_n + 1)
        co = np.array([int(c) * pow(shift_inv, k, P) % P for k, c in enumerate(co)], dtype=np.uint64)
        chunks[2 * i], chunks[2 * i + 1] = co[:n], co[n:]
    assert (_oracle.Batch(chunks, log_n, from_coeffs=True).cap.reshape(-1) == caps[2]).all(), "not the quotient the oracle's proof commits to"
