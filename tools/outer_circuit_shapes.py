#!/usr/bin/env python3
"""Pins the shape of the outer prover's statement circuits (sipp_amd/merkle.py, fri_fold.py, fri_initial.py): sha256 digests of everything
a circuit hands to the prover, for the shapes and inputs of tests/test_outer_circuit_pinned.py, which imports digests() from here.

    python tools/outer_circuit_shapes.py        # writes tests/golden/outer_circuit_shapes.json
    python tools/outer_circuit_shapes.py --mds  # writes tests/golden/plonk_vanishing_mds_shapes.json (tests/test_plonk_vanishing_mds.py)

Regenerate only when a circuit is meant to change, and say which entries moved and why."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "outer_circuit_shapes.json")
MDS_PATH = os.path.join(ROOT, "tests", "golden", "plonk_vanishing_mds_shapes.json")


def _sha(*parts):
    """arrays as little-endian 64-bit words behind their shape, everything else as JSON"""
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(json.dumps(list(p.shape)).encode())
            h.update(np.ascontiguousarray(p).astype("<i8" if p.dtype.kind == "i" else "<u8").tobytes())
        else:
            h.update(json.dumps(p, sort_keys=True).encode())
    return h.hexdigest()


def _ints(x):
    return [_ints(v) for v in x] if isinstance(x, (list, tuple)) else int(x)


def digests(c, witness_args, public_args, sigma_rows=True):
    """{item: sha256} of circuit c.  Canonical forms: the copy pairs sorted within each level, the cycles as a sorted list of sorted
    lists.  sigma_rows = False leaves the sigma rows out: the partition ("cycles") then stands for them."""
    circ, s, cs = c.circuit(), c.schedule(), c.constants_sigmas()
    k = circ["num_constants"]
    pairs = []
    for lv in range(s["n_levels"]):
        lo, hi = int(s["copy_offsets"][lv]), int(s["copy_offsets"][lv + 1])
        pairs.append(sorted(zip(_ints(list(s["copy_src"][lo:hi])), _ints(list(s["copy_dst"][lo:hi])))))
    assert int(s["copy_offsets"][-1]) == len(s["copy_src"]) == len(s["copy_dst"]) and cs.shape == (k + c.num_routed, c.n)
    out = {"circuit": _sha({key: v for key, v in circ.items() if key not in ("programs", "gates")}, _ints(circ["gates"]),
                           np.asarray(circ["programs"])),
           "generators": _sha(_ints(c.generators())),
           "constants": _sha(cs[:k], c.gate),
           "rows": _sha(c.log_n, c.n, c.rows_used, {name: _ints(v) for name, v in vars(c).items() if name.endswith("_row")}),
           "levels": _sha(c.n_levels, s["n_levels"], c.row_level, s["row_level"], s["rows"], s["level_offsets"], s["copy_offsets"]),
           "copies": _sha(pairs),
           "cycles": _sha(sorted(sorted(_ints(cyc)) for cyc in c.cycles)),
           "pi_cycle": _sha([sorted(_ints(cyc)) for cyc in c.pi_cycle]),
           "public_inputs": _sha(_ints(c.public_inputs(*public_args))),
           "partial_witness": _sha(c.partial_witness(*witness_args))}
    if sigma_rows:
        out["sigmas"] = _sha(cs[k:])
    return out


def main_mds():
    """the vanishing circuit's routed shapes (poseidon_mds, alpha_chunk) of tests/test_plonk_vanishing_mds.py, each with its counts"""
    sys.path.insert(0, ROOT)
    from tests import test_plonk_vanishing_mds as t
    out = {name: t.shape_digests(name) for name in t.PINNED}
    json.dump(out, open(MDS_PATH, "w"), indent=1, sort_keys=True)
    print("%d shapes -> %s" % (len(out), MDS_PATH))


def main():
    if "--mds" in sys.argv[1:]:
        return main_mds()
    sys.path.insert(0, ROOT)
    from tests import test_outer_circuit_pinned as t
    out = {t.name(kind, shape): t.shape_digests(kind, shape) for kind, shape in t.SHAPES}
    json.dump(out, open(PATH, "w"), indent=1, sort_keys=True)
    print("%d shapes -> %s" % (len(out), PATH))


if __name__ == "__main__":
    main()
