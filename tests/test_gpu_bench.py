"""bench.py's plain run: the headline line alone, exactly --steps timed steps, and --dump-outputs writing the three proofs of the
last timed step -- word for word the oracle's proofs of the n = 128 fixture (tests/golden/proof_digests_n128.json)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_bench_line_and_dumped_proofs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=500, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["unit"] == "pairings/s" and r["higher_is_better"] is True and r["dtype"] == "u64"
    assert abs(r["value"] - 128 / (r["ms_per_step"] * 1e-3)) / r["value"] < 1e-6
    # what only --full measures or checks is not in a plain line
    for k in ("verified", "kernel_ms_per_step", "pipelined", "cpu_baseline", "io_sharded", "outer_plonk", "native_chain"):
        assert k not in r, k
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests_n128.json")))
    for name, key, words in zip(("g1", "g2", "fq12"), ("g1_hardened", "g2_hardened", "fq12"), r["proof_words"]):
        a = np.load(str(tmp_path / ("proof_%s.npy" % name)))
        assert a.dtype == np.float64 and a.shape == (words, 2)
        assert (a == np.floor(a)).all() and a.min() >= 0 and a.max() < 2.0**32
        pf = a[:, 0].astype(np.uint64) | (a[:, 1].astype(np.uint64) << np.uint64(32))
        assert len(pf) == gold[key]["words"] and hashlib.sha256(pf.tobytes()).hexdigest() == gold[key]["sha256"], name
