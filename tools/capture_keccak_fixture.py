"""Writes tests/golden/keccak_proof_small.npz on a GPU: the proof of tools/capture_blinding_fixture.py -- the catalogue's circuit with lookups
and blinding rows (tests/_blinding_cases.py BlindCircuit: log_n = 10, rate_bits 3, cap height 4, 2 queries, three rounds of arity 4) under
(SEED, counter 0) -- with every Merkle tree hashed by Keccak-256 truncated to 25 bytes (CircuitProver(hasher="keccak")), and the
constants_sigmas cap the verifier needs.  tests/test_keccak_reading.py verifies it on the CPU.

    python tools/capture_keccak_fixture.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INPUTS = (9, 12)                 # a, b; the public input is xor4[16 a + b] = 5


def main(out):
    import sipp_amd
    from sipp_amd.circuit import CircuitProver
    from tests import _blinding_cases as bc
    c = bc.circuit(True)
    gp = sipp_amd.PlonkParams(c.num_routed, 8, 2)
    ctx = sipp_amd.Ctx(workspace_bytes=1 << 30)
    try:
        pr = CircuitProver(ctx, c, fri=bc.proof_fri(c.log_n, 0), params=gp, digest=bc.PROOF_DIGEST, zero_knowledge=True, seed=bc.SEED,
                           hasher="keccak")
        try:
            y = c.value(*INPUTS)
            proof = pr.prove(y, *INPUTS)
            cap = pr.cap.copy()
            assert pr.verify(proof) == (0, 0)
            assert int(proof[13]) == 1
        finally:
            pr.close()
    finally:
        ctx.close()
    np.savez_compressed(out, proof=proof, cap=cap, inputs=np.array(INPUTS, dtype=np.uint64), seed=np.array(bc.SEED, dtype=np.uint64))
    print("wrote %s: %d proof words" % (out, len(proof)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "keccak_proof_small.npz"))
