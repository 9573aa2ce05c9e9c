"""sipp::CircuitData::set_input_map / prove_words (include/sipp_host.hpp) through tests/host/test_circuit_words.cpp: the `basic` circuit
as data, its map and words in a file; the proof the program writes is the Python binding's sipp_circuit_prove_inputs proof word for
word, under the digest the library derives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests._basic_circuit import BasicCircuit
from tests.test_gpu_fri_generic import to_params
from tests.test_oracle_plonk import fri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIS, INDEX = [9, 1, 2, 3, 4], 3


def compile_host_program(tmp_path):
    import sipp_amd
    sipp_amd.lib()
    exe = str(tmp_path / "test_circuit_words")
    lib = os.path.join(ROOT, "sipp_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_circuit_words.cpp"), "-L" + lib, "-lsipp_hip", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_the_host_program_compiles(tmp_path):
    assert os.path.exists(compile_host_program(tmp_path))


@pytest.mark.gpu
def test_prove_words_cpp_is_the_python_bindings_proof(tmp_path):
    import sipp_amd
    exe = compile_host_program(tmp_path)
    circ = BasicCircuit()
    ofp = fri(circ.log_n, rate_bits=3, cap_height=4, nq=8, arity=4, fpb=4)
    gfp, gp, cd = to_params(ofp), sipp_amd.PlonkParams(80, 8, 2), circ.circuit()
    cells, vals = circ.input_cells(PIS, INDEX)
    pis = circ.public_inputs(PIS)
    rng = np.random.default_rng(7)
    n_words, n_extra = 40, 9
    staged = rng.integers(0, 1 << 63, size=n_words + n_extra, dtype=np.uint64)
    sources = rng.permutation(n_words + n_extra)[:len(vals)].astype(np.uint64)
    staged[sources.astype(np.int64)] = vals
    sc, gens, cs = circ.schedule(), circ.generators(), circ.constants_sigmas()
    u64 = lambda v: np.ascontiguousarray(v, dtype=np.uint64).reshape(-1)
    head = [circ.log_n, cd["num_wires"], cd["num_routed"], cd["num_constants"], cd["num_selectors"], len(cd["gates"]), len(cd["programs"]), len(gens),
            sc["n_levels"], len(sc["rows"]), len(sc["copy_src"]), len(pis), 8, len(cells), n_words, n_extra]
    fp_words = [gfp.rate_bits, gfp.cap_height, gfp.pow_bits, gfp.num_queries, gfp.pow_rule, gfp.hiding, gfp.n_rounds] + [int(x) for x in gfp.arity_bits]
    parts = [u64(head), u64(fp_words), u64([list(g) for g in cd["gates"]]), cd["programs"].astype(np.int64).view(np.uint64), u64([list(g) for g in gens]),
             u64(sc["rows"]), u64(sc["level_offsets"]), u64(sc["copy_src"]), u64(sc["copy_dst"]), u64(sc["copy_offsets"]), u64(cs), cells, sources,
             staged[:n_words], staged[n_words:], u64(pis)]
    with open(tmp_path / "fixture.bin", "wb") as f:
        for a in parts:
            f.write(a.tobytes())
    out = subprocess.run([exe, str(tmp_path / "fixture.bin"), str(tmp_path / "proof.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "prove_words ok" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(tmp_path / "proof.bin", dtype=np.uint64)
    pf, digest = got[:-4], [int(x) for x in got[-4:]]
    gc = sipp_amd.PlonkCircuit.from_dict(cd)
    ctx = sipp_amd.Ctx(workspace_bytes=sipp_amd.lib().sipp_circuit_workspace_bytes(circ.log_n, C.byref(gp), C.byref(gfp), C.byref(gc)))
    try:
        data = sipp_amd.CircuitData(ctx, circ.log_n, gp, gfp, gc, cs, gens, sched=sc)
        assert [int(x) for x in data.digest] == digest
        want = data.prove_inputs(cells, vals, pis)
        assert len(pf) == len(want) and (pf == want).all() and data.verify(pf) == (0, 0)
        data.close()
    finally:
        ctx.close()
