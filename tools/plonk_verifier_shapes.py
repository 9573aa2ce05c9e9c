#!/usr/bin/env python3
"""Pins the shape of the one-circuit verifier (sipp_amd/plonk_verifier.py) for the cases of tests/test_plonk_verifier_circuit.py, which
owns shape_digests(): per case the counts (rows used, log_n, levels, public inputs, witness inputs, input cells, generators) and the
sha256 digests tools/outer_circuit_shapes.py takes of everything a circuit hands to the prover.

    python tools/plonk_verifier_shapes.py       # writes tests/golden/plonk_verifier_shapes.json

Regenerate only when the circuit is meant to change, and say which entries moved and why."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "plonk_verifier_shapes.json")


def main():
    sys.path.insert(0, ROOT)
    from tests import test_plonk_verifier_circuit as t
    out = {case: t.shape_digests(case) for case in sorted(t.CASES)}
    json.dump(out, open(PATH, "w"), indent=1, sort_keys=True)
    print("%d shapes -> %s" % (len(out), PATH))


if __name__ == "__main__":
    main()
