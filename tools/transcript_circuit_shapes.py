#!/usr/bin/env python3
"""Pins the shape of the transcript circuit (sipp_amd/transcript.py) at n = 4 and n = 8 over the fixtures of tests/golden: per size the
counts (rows used, log_n, levels, public inputs, witness inputs, input cells, generators, transcript rows) and the sha256 digests
tools/outer_circuit_shapes.py takes of everything a circuit hands to the prover.  tests/test_transcript_circuit.py owns shape_digests().

    python tools/transcript_circuit_shapes.py       # writes tests/golden/transcript_circuit_shapes.json

Regenerate only when the circuit is meant to change, and say which entries moved and why."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "transcript_circuit_shapes.json")


def main():
    sys.path.insert(0, ROOT)
    from tests import test_transcript_circuit as t
    out = {"n%d" % n: t.shape_digests(n) for n in t.SIZES}
    json.dump(out, open(PATH, "w"), indent=1, sort_keys=True)
    print("%d shapes -> %s" % (len(out), PATH))


if __name__ == "__main__":
    main()
