#!/usr/bin/env python3
"""Pins the shape of the whole FRI verifier circuit (sipp_amd/fri_proof.py) as tools/fri_verifier_circuit_shapes.py pins the query-round
circuit: tools/outer_circuit_shapes.py's digests() over the shapes and the fixed inputs of tests/test_fri_proof_circuit.py.

    python tools/fri_proof_circuit_shapes.py        # writes tests/golden/fri_proof_circuit_shapes.json

Regenerate only when the circuit is meant to change, and say which entries moved and why."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    from tests import test_fri_proof_circuit as t
    out = {name: t.shape_digests(name) for name in t.PINNED}
    json.dump(out, open(t.GOLDEN, "w"), indent=1, sort_keys=True)
    print("%d shapes -> %s" % (len(out), t.GOLDEN))


if __name__ == "__main__":
    main()
