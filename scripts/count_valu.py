#!/usr/bin/env python3
"""Static instruction counts of a .hip file's kernels: compiles it to gfx950 assembly with the flags READ from sipp_amd/csrc/Makefile and prints, per
kernel, the v_* instructions, the s_nop wait states (each s_nop N counts N + 1), VGPRs, scratch bytes and occupancy as the compiler
reports them.  Counts are per lane and STATIC (every instruction of the kernel's text once, loops not multiplied out): they compare two
spellings of the same kernel, they are not the dynamic counts of profiles/*_valu_by_kernel.json.

    scripts/count_valu.py sipp_amd/csrc/ntt_tree.hip [--filter tree_] [-D NAME=VALUE ...]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags():
    """the flags the library's device code is compiled with, read from sipp_amd/csrc/Makefile (HIPFLAGS and what the %.o: %.hip rule
    adds between $(HIPFLAGS) and -c), so that the counts are those of the code as it ships"""
    csrc = os.path.join(ROOT, "sipp_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", text, flags=re.M).group(1).split()
    flags += re.search(r"^\t\$\(HIPCC\) \$\(HIPFLAGS\) (.*?) -c \$<", text, flags=re.M).group(1).split()
    arch = re.search(r"^ARCH \?= (\S+)", text, flags=re.M).group(1)
    out, i = [], 0
    while i < len(flags):
        f = flags[i].replace("$(ARCH)", arch)
        if f == "-I":                                  # include paths of the Makefile are relative to csrc
            out += ["-I", os.path.normpath(os.path.join(csrc, flags[i + 1]))]
            i += 2
            continue
        out.append(f)
        i += 1
    return out


def compile_to_asm(src, defines, hipcc):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        cmd = [hipcc] + makefile_flags() + ["-I", os.path.join(ROOT, "sipp_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                                            "--cuda-device-only", "-S", src, "-o", out] + ["-D" + d for d in defines]
        subprocess.run(cmd, check=True)
        with open(out) as f:
            return f.read()


def kernels(asm):
    """yields (name, text) per kernel: from the label `name:` to the end of the compiler's "Kernel info" comment behind it"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?;\s*Occupancy:\s*\d+)" % re.escape(name), asm, flags=re.M | re.S)
        if m:
            yield name, m.group(1)


def count(body):
    valu = nops = 0
    for line in body.splitlines():
        ins = line.split(";")[0].strip()
        if not ins or ins.startswith(".") or ins.endswith(":"):
            continue
        op = ins.split()[0]
        if op.startswith("v_"):
            valu += 1
        elif op == "s_nop":
            nops += int(ins.split()[1], 0) + 1

    def field(pat, default="?"):
        m = re.search(pat, body)
        return m.group(1) if m else default
    return dict(valu=valu, s_nop=nops, vgprs=field(r"\.amdhsa_next_free_vgpr\s+(\d+)"), scratch=field(r";\s*ScratchSize:\s*(\d+)"),
                occupancy=field(r";\s*Occupancy:\s*(\d+)"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("--filter", default="", help="only kernels whose (mangled) name contains this")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    asm = compile_to_asm(args.source, args.defines, args.hipcc)
    print("%-72s %7s %6s %6s %8s %4s" % ("kernel", "VALU", "s_nop", "VGPRs", "scratch", "occ"))
    for name, body in kernels(asm):
        if args.filter not in name:
            continue
        c = count(body)
        print("%-72s %7d %6d %6s %8s %4s" % (name[:72], c["valu"], c["s_nop"], c["vgprs"], c["scratch"], c["occupancy"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
