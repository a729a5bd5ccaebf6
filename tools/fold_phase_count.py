#!/usr/bin/env python3
"""Static instruction count of k_embed_fold per phase, from the device assembly (no GPU needed).
    python tools/fold_phase_count.py [--source FILE] [--kernel 'k_embed_fold<2, 5, 8, true, false>']
The kernel's phase stamps (AZK_FSTAMP, empty in a product build) are compiled as assembly comments in a copy of the source, the copy
is compiled like the product (-O3 -fno-slp-vectorize, device only), and the instructions between the marks are counted in text order
by class.  --source: another version of azk_nn.hip (e.g. `git show HEAD~1:alpha-zero_amd/csrc/azk_nn.hip > /tmp/old.hip`), compiled
against this tree's headers.  The count is static: a block that the benched shape never enters (the flag words 2 - 4 of a thread at
more than 2 048 games, the boards of more than 512 cells) counts like any other, and is listed so that it can be set aside."""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alpha-zero_amd", "csrc")
EMPTY = "#define AZK_FSTAMP(i) do { } while (0)"
PHASES = ["launch prologue", "board load + bit string", "patch bits + compaction", "gather + tile loop", "ticket, sums, output rows", "after the board loop"]


def classify(op):
    if "mfma" in op:
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_load", "s_buffer_load")):
        return "wait/sload"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "VMEM"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=os.path.join(CSRC, "azk_nn.hip"))
    ap.add_argument("--kernel", default="k_embed_fold<2, 5, 8, true, false>")
    ap.add_argument("--blocks", action="store_true", help="also list every basic block")
    a = ap.parse_args()
    text = open(a.source).read()
    assert EMPTY in text, "the empty AZK_FSTAMP definition was not found"
    text = text.replace(EMPTY, '#define AZK_FSTAMP(i) asm volatile("; azk_phase " #i)')
    with tempfile.TemporaryDirectory() as td:
        src, out = os.path.join(td, "azk_nn_marks.hip"), os.path.join(td, "dev.s")
        open(src, "w").write(text)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-fno-slp-vectorize", "--offload-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL)
        asm = open(out).read().splitlines()
    labels = [m.group(1) for m in (re.match(r"^(_Z\w+):", l) for l in asm) if m]
    names = subprocess.run(["c++filt"], input="\n".join(labels), capture_output=True, text=True).stdout.splitlines()
    want = [m for m, n in zip(labels, names) if a.kernel.replace(" ", "") in n.replace(" ", "")]
    assert len(want) == 1, (a.kernel, want)
    start = next(i for i, l in enumerate(asm) if l.startswith(want[0] + ":"))
    phase, block = 0, "entry"
    per_phase = [collections.Counter() for _ in PHASES]
    per_block = collections.OrderedDict()
    for l in asm[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            block = m.group(1)
            continue
        m = re.match(r"^; azk_phase (\d)", t)
        if m:
            phase = int(m.group(1)) + 1
            continue
        if not t or t.startswith((";", ".")):
            continue
        c = classify(t.split()[0])
        per_phase[phase][c] += 1
        per_block.setdefault((phase, block), collections.Counter())[c] += 1
    cols = ["VALU", "SALU", "MFMA", "LDS", "VMEM", "branch", "wait/sload"]
    print(a.kernel, "from", a.source)
    print("%-28s" % "phase" + "".join("%11s" % c for c in cols))
    for name, cnt in zip(PHASES, per_phase):
        print("%-28s" % name + "".join("%11d" % cnt[c] for c in cols))
    tot = sum(per_phase, collections.Counter())
    print("%-28s" % "all" + "".join("%11d" % tot[c] for c in cols))
    loop = [(k, v) for k, v in per_block.items() if v["MFMA"]]
    print("tile loop body (the blocks with MFMAs): " + ", ".join("%s %d" % (c, sum(v[c] for _, v in loop)) for c in cols[:5]))
    if a.blocks:
        for (ph, b), v in per_block.items():
            print("  phase %d %-12s" % (ph, b) + " ".join("%s %d" % (c, v[c]) for c in cols if v[c]))


if __name__ == "__main__":
    main()
