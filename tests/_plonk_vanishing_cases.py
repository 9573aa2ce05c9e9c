"""The inner circuits of the vanishing-circuit tests, each at the smallest log_n its FRI parameters admit and with 8 queries:

  basic      tests/_basic_circuit.py: Constant, PublicInput, BaseSum, RandomAccess and arithmetic rows, two selector columns; R = 80, D = 8, C = 2
  ragged     the same gates under ONE selector column (no UNUSED factor), R = 67: the last chunk has 3 wires; C = 1
  poseidon   MerkleOpeningCircuit(3, 1, 1, 1): the Poseidon gate's 123 constraints, negative coefficients, pih factors, shared S-box powers

inner(name) -> what a test needs of one: the circuit, its constants_sigmas and their cap, the replayed witness, the public inputs, the
parameters (R, D, C) with the oracle's structs.  The inner PROOF is the caller's: the oracle's on the CPU, the device's on the GPU."""
import numpy as np

from sipp_amd import merkle as mk
from tests import _oracle
from tests import _witness_reading as rd
from tests._basic_circuit import BasicCircuit
from tests.test_oracle_plonk import fri

NAMES = ("basic", "ragged", "poseidon")
INNER_DIGEST = (21, 22, 23, 24)
CAP_HEIGHT = 4
_made = {}


def inner(name):
    if name in _made:
        return _made[name]
    if name == "poseidon":
        from oracle.py import plonky2_generic as g2
        c, params = mk.MerkleOpeningCircuit(3, 1, 1, 1), (80, 8, 2)
        leaves = [[5, 6, 7], [8, 9, 10], [11, 12, 13], [14, 15, 16]]
        tree = g2.MerkleTree(leaves, 1)
        args = ([v for d in tree.cap for v in d], [3], [leaves[3]], [tree.prove(3)])
        pis, pw = c.public_inputs(*args[:3]), c.partial_witness(*args)
    else:
        c = BasicCircuit() if name == "basic" else BasicCircuit(num_routed=67, groups=(0,) * 6)
        params = (80, 8, 2) if name == "basic" else (67, 8, 1)
        args = ([13, 3, _oracle.P - 1, 5, 1 << 40], 2)
        pis, pw = c.public_inputs(args[0]), c.partial_witness(*args)
    cs = c.constants_sigmas()
    pih = _oracle.hash_no_pad(np.array(pis, dtype=np.uint64))
    w = rd.replay(pw, cs[:c.num_constants], c.generators(), pih, c.schedule())
    _made[name] = {"name": name, "c": c, "circ": c.circuit(), "cs": cs, "w": w, "pw": pw, "pis": [int(v) for v in pis], "params": params,
                   "op": _oracle.plonk_params(*params), "ofp": fri(c.log_n, rate_bits=3, cap_height=CAP_HEIGHT, nq=8, arity=4, fpb=4),
                   "cap": _oracle.Batch(cs, c.log_n, rate_bits=3, cap_height=CAP_HEIGHT).cap, "args": args}
    return _made[name]


def oracle_proof(o):
    """the inner proof by the oracle's prover, once"""
    if "proof" not in o:
        o["proof"] = _oracle.plonk_prove_gates(o["w"], o["cs"], o["c"].log_n, o["op"], o["ofp"], o["circ"], INNER_DIGEST, o["pis"])
    return o["proof"]
