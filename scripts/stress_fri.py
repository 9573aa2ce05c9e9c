#!/usr/bin/env python3
"""One-off stress run of the generic layer (GPU box): random FriParams (blowup 2 / 4 / 8, cap heights, constant or mixed arities
2 .. 16, final polynomial sizes, both proof-of-work rules, query counts), random numbers of oracles with random widths (1 .. 4
columns = unhashed leaves included), random salting, random batches of column ranges -- sipp_commit_batch_ex and
sipp_fri_prove_openings against oracle/fri.c word for word, then the oracle's verifier.
usage: stress_fri.py [first_seed=700] [count=40]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sipp_amd  # noqa: E402
from sipp_amd._lib import to_device  # noqa: E402
from tests import _oracle, _verify  # noqa: E402
from tests._fri_cases import stress_config, stress_data  # noqa: E402
from tests.test_gpu_fri_generic import gpu_challenger, to_params  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 700
count = int(sys.argv[2]) if len(sys.argv) > 2 else 40
ctx = sipp_amd.Ctx(workspace_bytes=4 << 30)
bad = skipped = declined = 0
t0 = time.time()
for seed in range(first, first + count):
    cfg, rng = stress_config(seed)       # tests/_fri_cases.py: the configuration as a function of the seed
    log_n, rate_bits, cap_height, fp, tag = cfg["log_n"], cfg["rate_bits"], cfg["cap_height"], cfg["fp"], cfg["tag"]
    try:
        oracles, batches = stress_data(cfg, rng)
        gch, och = gpu_challenger([seed, 1, 2])
        ref = _oracle.fri_prove_openings(oracles, batches, log_n, fp, och)
    except Exception as e:      # noqa: BLE001 -- a configuration the oracle itself refuses (e.g. cap higher than the last layer)
        skipped += 1
        print(tag + " -- oracle refuses: %s" % str(e)[:80], flush=True)
        continue
    try:
        devs, keep = [], []
        for k, o in enumerate(oracles):
            coeffs = o.coeffs
            if k % 2 == 0:
                vals = coeffs.copy()
                L = _oracle.load()
                for c in range(vals.shape[0]):
                    L.orc_fft(vals[c], log_n)
                data, from_coeffs = vals, False
            else:
                data, from_coeffs = coeffs, True
            salt = None if o.salt is None else to_device(o.salt)
            od, cap, bufs = ctx.commit_ex(to_device(data), log_n, rate_bits, cap_height, from_coeffs=from_coeffs, salt=salt)
            assert (cap == o.cap).all(), "cap of oracle %d" % k
            devs.append(od)
            keep.append(bufs)
        got = ctx.fri_prove_openings(devs, batches, log_n, to_params(fp), gch)
        ok = len(got) == len(ref) and bool((got == ref).all())
        ok = ok and [gch.state[i] for i in range(12)] == [och.state[i] for i in range(12)]
        ok = ok and _oracle.fri_verify_openings(got, [o.cap for o in oracles], [o.ncols for o in oracles], [o.n_salt for o in oracles],
                                                batches, log_n, fp, _oracle.challenger([seed, 1, 2])) == 0
        # ... and the library's own verifier (sipp_fri_verify_openings), transcript included
        lib_stage, lib_ch = _verify.lib_fri_verify(got, [o.cap for o in oracles], [o.ncols for o in oracles], [o.n_salt for o in oracles], batches, log_n, fp,
                                                   _oracle.challenger([seed, 1, 2]))
        ok = ok and lib_stage == 0 and lib_ch == bytes(och)
    except sipp_amd.SippError as e:
        if e.code == -7:        # SIPP_E_UNSUPPORTED: outside the documented range of the GPU layer (e.g. a layer of < 16 values)
            declined += 1
            print("declined " + tag + " -- %s" % str(e)[:90], flush=True)
            continue
        ok = False
        tag += " -- GPU: %s" % str(e)[:100]
    except AssertionError as e:
        ok = False
        tag += " -- GPU: %s" % str(e)[:100]
    if not ok:
        bad += 1
    print(("ok   " if ok else "MISMATCH ") + tag + " (%.0f s)" % (time.time() - t0), flush=True)
print("done: %d seeds, %d mismatches, %d refused by the oracle, %d declined by the GPU layer (unsupported range)" % (count, bad, skipped, declined))
sys.exit(1 if bad else 0)
