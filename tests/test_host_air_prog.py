"""air_read_gadgets (sipp_amd/csrc/air_prog.hpp), the one reading of the gadget part of an AIR program that the trace fill's gadget and
product tables and the quotient's segment table are built from, on the CPU: tests/host/air_prog.cpp compiles the header's own code (no
device) and, for every entry of AIR_AIRS, compares it with a second, bounds-checked walk written from the program format -- the gadget
count equals n_gadgets, every offset points at an op word 1 and the offsets increase strictly, every gadget has np + 1 product offsets
inside it, and the POLY ops walked from the reported start end exactly at prog_len.  Built twice into the test's temporary directory:
plain, and with AddressSanitizer + UBSan; both are stand-alone programs, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "air_prog.cpp")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return c
    pytest.fail("no C++ compiler for the host test")


def _n_airs():
    text = open(os.path.join(ROOT, "data", "air_tables.h")).read()
    return int(re.search(r"AIR_AIRS\[(\d+)\]", text).group(1))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "sanitized"])
def test_gadget_reading_matches_a_plain_walk(tmp_path, flags):
    exe = str(tmp_path / "air_prog")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-variable", "-Wno-unused-const-variable"] + flags +
                          ["-I", os.path.join(ROOT, "sipp_amd", "csrc"), "-I", os.path.join(ROOT, "data"), "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "air_prog ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    # every AIR was read, and the programs are not empty: gadgets, products and POLY ops were all met
    m = re.search(r"(\d+) airs, (\d+) gadgets, (\d+) products, (\d+) POLY ops, 0 failures", out.stdout)
    assert m, out.stdout
    airs, gadgets, products, polys = map(int, m.groups())
    assert airs == _n_airs() and gadgets >= airs and products > 0 and polys > 0, out.stdout
