"""gl::reduce6 (sipp_amd/csrc/gl.hpp), the two-chain reduction behind gl::Acc6::reduce, on the CPU: tests/host/lazy_reduce.cpp compiles
the header's own code (no device) and compares it with unsigned __int128 arithmetic mod p -- all zero, every accumulator at 2^60 - 1 (the
hash kernels' bound) and at 2^64 - 1 (Acc6's own contract), each accumulator and each 32-bit half alone at its maximum, the extremes of
the two chains, 10^5 seeded random sextuples.  Built twice into the test's temporary directory: plain, and with AddressSanitizer +
UBSan; both are stand-alone programs, nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "lazy_reduce.cpp")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return c
    pytest.fail("no C++ compiler for the host test")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "sanitized"])
def test_two_chain_reduction_matches_int128(tmp_path, flags):
    exe = str(tmp_path / "lazy_reduce")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "sipp_amd", "csrc"), "-o", exe, SRC])
    out = subprocess.run([exe, "100000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lazy_reduce ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    # 47 edge sextuples + the random ones: the program ran all of them
    assert "100047 sextuples, 0 mismatches" in out.stdout, out.stdout
