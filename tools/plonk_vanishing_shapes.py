#!/usr/bin/env python3
"""Pins the shape of the vanishing circuit (sipp_amd/plonk_vanishing.py) for the three inner circuits of
tests/_plonk_vanishing_cases.py: sha256 digests of everything the circuit hands to the prover (tools/outer_circuit_shapes.py's digests).

    python tools/plonk_vanishing_shapes.py        # writes tests/golden/plonk_vanishing_shapes.json

Regenerate only when the circuit is meant to change, and say which entries moved and why."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "plonk_vanishing_shapes.json")


def main():
    sys.path.insert(0, ROOT)
    from tests import _plonk_vanishing_cases as cases
    from tests import test_plonk_vanishing_circuit as t
    out = {name: t.shape_digests(name) for name in cases.NAMES}
    json.dump(out, open(PATH, "w"), indent=1, sort_keys=True)
    print("%d shapes -> %s" % (len(out), PATH))


if __name__ == "__main__":
    main()
