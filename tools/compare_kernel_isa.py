#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libazk.so kernel by kernel (no GPU needed):

    python3 tools/compare_kernel_isa.py OLD/libazk.so alpha-zero_amd/azk/libazk.so [--match k_tree]

Extracts each library's first code object (csrc/azk_engine.hip's: the tree and rule kernels), disassembles it with llvm-objdump and
compares the instruction text of every kernel symbol whose name contains --match (addresses and encodings left out).  Exit status 1
if any such kernel differs or is missing.  This is how "k_tree's instruction stream did not change" is checked for a change that
must leave parity mode alone."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")      # ROCm's own default install prefix


def kernels(so, work, tag):
    fat, co = os.path.join(work, tag + ".fatbin"), os.path.join(work, tag + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.strip():
            out[cur].append(line.split("//")[0].strip())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="k_tree")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        old, new = kernels(a.old, work, "old"), kernels(a.new, work, "new")
    names = sorted(k for k in old if a.match in k)
    if not names:
        print("no kernel matches", a.match)
        return 1
    bad = 0
    for k in names:
        same = old[k] == new.get(k)
        bad += not same
        print("same" if same else "DIFFERENT", len(old[k]), "instructions", k)
    print("only in the new build:", sorted(k for k in new if k not in old))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
