"""From the points A, B of a SIPP instance to its three STARK proofs on one GPU: what each road costs.

    perf_flow.py n [count] [in_flight] [--passes P] [--reps R] [--native-priority LEVEL] [--stages-only]

After two warm-up rounds the variants alternate within this process, P passes of R repetitions each; a pass's figure is the mean of its
repetitions, and the line printed per variant gives the minimum, the median and the maximum over the passes (max - min = the run-to-run
spread).  Variants:
    prove_native, verify_native, Instance.prove     stage by stage (their sum is the stage-by-stage flow)
    prove_native_ex                                 the one-pass native chain, all outputs
    flow                                            Instance.flow: one instance, native chain then proofs
    queued proofs                                   InstanceQueue.prove on lists that exist already, per instance
    queued flow                                     InstanceQueue.flows: the producer's native chains beside the proofs, per instance
A library without sipp_prove_native_ex (an earlier build) is measured stage by stage and queued only: the same script gives the
figures to compare against; --stages-only measures this build the same way (the same load between the timed calls).  --native-priority
1 / 0 / -1 puts the native chain's ctx on a high-priority stream / a stream with a queue of its own (default) / see
sipp_ctx_set_stream_priority.  Every proof goes through sipp_stark_verify after the timed region.  The last line is one JSON object."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sipp_amd  # noqa: E402
from sipp_amd import _lib  # noqa: E402


def main():
    argv = sys.argv[1:]
    opt = {"--passes": 5, "--reps": 3, "--native-priority": 0}
    stages_only = "--stages-only" in argv
    if stages_only:
        argv.remove("--stages-only")
    for name in list(opt):
        if name in argv:
            i = argv.index(name)
            opt[name] = int(argv[i + 1])
            del argv[i: i + 2]
    n = int(argv[0]) if argv else 128
    count = int(argv[1]) if len(argv) > 1 else 6
    in_flight = int(argv[2]) if len(argv) > 2 else 3
    passes, reps = opt["--passes"], opt["--reps"]
    has_ex = "sipp_prove_native_ex" in _lib.SIGNATURES and not stages_only

    st = np.load(os.path.join(ROOT, "tests", "golden", "sipp_n%d_ios.npz" % n))["statement"]
    A = np.ascontiguousarray(st[: 16 * n].reshape(n, 16), dtype=np.uint32)
    B = np.ascontiguousarray(st[16 * n: 48 * n].reshape(n, 32), dtype=np.uint32)
    lg = n.bit_length() - 1
    num_io = [n - 1, n - 1, 2 * lg]
    # the queue's instances: the fixture with its pairs rolled (different points in every place, the same product)
    points = [(np.ascontiguousarray(np.roll(A, k, axis=0)), np.ascontiguousarray(np.roll(B, k, axis=0))) for k in range(count)]

    L = sipp_amd.lib()
    nctx = sipp_amd.Ctx(workspace_bytes=max(1 << 30, L.sipp_workspace_bytes(1, max(1, n // 2)), L.sipp_workspace_bytes(2, max(1, 2 * lg))))
    if opt["--native-priority"]:
        nctx._ck(L.sipp_ctx_set_stream_priority(nctx.h, opt["--native-priority"]), "set_stream_priority")
    inst = sipp_amd.Instance(num_io)
    queue = sipp_amd.InstanceQueue(num_io, in_flight=in_flight)
    lists = []
    for a, b in points:
        ok, _, ios = nctx.verify_native(a, b, nctx.prove_native(a, b))
        assert ok
        lists.append(ios)
    proof0 = nctx.prove_native(A, B)
    to_verify = []

    def keep(proofs):
        to_verify.append([p.copy() for p in proofs])

    def v_prove_native():
        nctx.prove_native(A, B)

    def v_verify_native():
        assert nctx.verify_native(A, B, proof0)[0]

    def v_instance_prove():
        return inst.prove(lists[0])

    def v_ex():
        assert nctx.prove_native_ex(A, B)[1]

    def v_flow():
        return inst.flow(nctx, A, B)[0]

    def v_queued_proofs():
        return queue.prove(lists)

    def v_queued_flow():
        return [r[0] for r in queue.flows(nctx, points)]

    variants = [("prove_native", v_prove_native, 1), ("verify_native", v_verify_native, 1), ("instance_prove", v_instance_prove, 1)]
    if has_ex:
        variants += [("prove_native_ex", v_ex, 1), ("flow", v_flow, 1)]
    variants.append(("queued_proofs", v_queued_proofs, count))
    if has_ex:
        variants.append(("queued_flow", v_queued_flow, count))

    for _ in range(2):                                    # warm-up: every variant, untimed
        for _, fn, _ in variants:
            fn()
    ms = {name: [] for name, _, _ in variants}
    for p in range(passes):
        for name, fn, per in variants:
            t = time.perf_counter()
            for _ in range(reps):
                out = fn()
            ms[name].append(1e3 * (time.perf_counter() - t) / reps / per)
            if p == passes - 1 and out is not None:       # what the last timed call produced is what gets verified
                if name in ("queued_proofs", "queued_flow"):
                    for proofs in out:
                        keep(proofs)
                else:
                    keep(out)
    verified = 0
    for proofs in to_verify:                              # after the timed region
        for pf in proofs:
            assert sipp_amd.stark_verify(pf) == 0, "sipp_stark_verify refuses a proof"
            verified += 1

    summary = {name: {"min": round(min(v), 2), "median": round(statistics.median(v), 2), "max": round(max(v), 2)} for name, v in ms.items()}
    stage = [sum(x) for x in zip(ms["prove_native"], ms["verify_native"], ms["instance_prove"])]
    native2 = [sum(x) for x in zip(ms["prove_native"], ms["verify_native"])]
    summary["prove_plus_verify_native"] = {"min": round(min(native2), 2), "median": round(statistics.median(native2), 2), "max": round(max(native2), 2)}
    summary["stage_by_stage_flow"] = {"min": round(min(stage), 2), "median": round(statistics.median(stage), 2), "max": round(max(stage), 2)}
    print("n = %d, %d passes x %d repetitions, queue of %d instances through %d slots; ms (per instance for the queues): min / median / max"
          % (n, passes, reps, count, in_flight))
    for name, s in summary.items():
        print("  %-26s %8.2f %8.2f %8.2f" % (name, s["min"], s["median"], s["max"]))
    print("  %d proofs accepted by sipp_stark_verify" % verified)
    print(json.dumps({"n": n, "count": count, "in_flight": in_flight, "passes": passes, "reps": reps, "has_prove_native_ex": has_ex,
                      "native_priority": opt["--native-priority"],
                      "ms": summary, "per_pass_ms": {k: [round(x, 2) for x in v] for k, v in ms.items()}, "proofs_verified": verified}))
    queue.close()
    inst.close()
    nctx.close()


if __name__ == "__main__":
    main()
