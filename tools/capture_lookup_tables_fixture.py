"""Writes tests/golden/lookup_tables_proof_small.npz on a GPU: one "SIPPPLK4" proof with two tagged tables (description word 7 != 0)
of the zero-constraint circuit over the tagged catalogue's largest entry (tests/_lookup_tables_cases.py PROOF_ENTRY: log_n = 10, with
tests/_lookup_cases.py's PROOF_* parameters: rate_bits 3, cap height 4, 8 queries) and the constants_sigmas cap the verifier needs.
tests/test_lookup_tables_reading.py verifies it on the CPU.

    python tools/capture_lookup_tables_fixture.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import sipp_amd
    from sipp_amd.circuit import fri_params
    from sipp_amd._lib import to_device
    from tests import _lookup_cases as lc
    from tests import _lookup_tables_cases as tc
    e = tc.BY_NAME[tc.PROOF_ENTRY]()
    ctx = sipp_amd.Ctx(workspace_bytes=1 << 30)
    try:
        cs = to_device(lc.constants_sigmas(e))
        circ = sipp_amd.PlonkCircuit.from_dict(lc.proof_circuit(e))
        gp = sipp_amd.PlonkParams(lc.PROOF_ROUTED, e["D"], e["C"])
        fp = fri_params(e["log_n"], **lc.PROOF_FRI)
        _, cap, _keep = ctx.commit_ex(cs, e["log_n"], fp.rate_bits, fp.cap_height)
        wires = ctx.plonk_lookup_multiplicities(to_device(e["wires"]), cs[: e["consts"].shape[0]].contiguous(), e["log_n"], e["num_selectors"], e["desc"])
        proof = ctx.plonk_prove_gates_lookup(wires, cs, e["log_n"], gp, fp, circ, lc.PROOF_DIGEST, [], e["desc"])
    finally:
        ctx.close()
    assert sipp_amd.plonk_verify_gates_lookup(proof, cap, gp, fp, circ, lc.PROOF_DIGEST, e["desc"]) == 0
    np.savez_compressed(out, proof=proof, cap=cap, entry=np.array(tc.PROOF_ENTRY))
    print("wrote %s: %d proof words" % (out, len(proof)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lookup_tables_proof_small.npz"))
