#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libazk.so kernel by kernel (no GPU needed):

    python3 tools/compare_kernel_isa.py OLD/csrc/build alpha-zero_amd/csrc/build [--match k_tree]
    python3 tools/compare_kernel_isa.py OLD/libazk.so alpha-zero_amd/azk/libazk.so
    python3 tools/compare_kernel_isa.py OLD/csrc/build alpha-zero_amd/csrc/build --strip-namespace azk_eng
    python3 tools/compare_kernel_isa.py OLD/csrc/build alpha-zero_amd/csrc/build --strip-namespace azk_eng --rename profiles/mover_options_rename.tsv

Each side is a build directory (every *.o in it) or a library.  Every code object bundled in them is extracted (one per translation
unit: csrc/azk_search.hip, azk_begin.hip, azk_moves.hip, azk_nn.hip, ...), every kernel is cut at its symbol's size (llvm-readelf -s: llvm-objdump -d goes on to
disassemble a section's padding as if it were code) and the instruction text is compared symbol by symbol, whichever file the
symbol lives in on either side (addresses and encodings left out; kernels in anonymous namespaces keep their mangled names when
they move between files).  A mangled name also spells the namespaces of the kernel's parameter types, so a type that moves to
another namespace renames every kernel that takes it: --strip-namespace NS (repeatable) compares by DEMANGLED name instead
(c++filt), with the qualifiers `NS::` and `(anonymous namespace)::` taken out on both sides; two kernels of one build that
fall onto the same name that way are an error, never a silent pairing.  --rename FILE (only with --strip-namespace) pairs kernels whose
names changed on purpose: each line of FILE is `old demangled name<TAB>new demangled name`, both as the stripped comparison prints them,
and the OLD side is renamed before pairing; a line that names no old kernel, or two old kernels that end on one name, are errors.  A kernel
that differs is printed with the instruction counts of both sides.  The 64-byte kernel descriptors (register counts, LDS size, ...) are compared too, less the code's own
offset.  --match keeps the kernels whose name contains the string.  Exit status 1 if a kernel differs, is missing or is new.  This is
how "k_tree's instruction stream did not change"  and "moving code between files left the device code alone"
 are checked."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")      # ROCm's own default install prefix
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def tool(name, *args, **kw):
    return subprocess.check_output([os.path.join(LLVM, name), *args], **kw)


def code_objects(path, work, tag):
    """The gfx950 code objects of a build directory's objects or of a library, as files under work."""
    files = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
    if not files:
        sys.exit("no object files in " + path)
    out = []
    for f in files:
        fat = os.path.join(work, "%s%d.fatbin" % (tag, len(out)))
        tool("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", f, fat)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]         # a library holds one bundle per translation unit
        for lo, hi in zip(starts, starts[1:] + [len(blob)]):
            one, co = os.path.join(work, "%s%d.bundle" % (tag, len(out))), os.path.join(work, "%s%d.co" % (tag, len(out)))
            open(one, "wb").write(blob[lo:hi])
            tool("clang-offload-bundler", "--type=o", "--input=" + one, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co,
                 "--unbundle")
            out.append(co)
    return out


def kernels(path, work, tag):
    """{kernel symbol: (instruction lines within the symbol's size, descriptor bytes)} over every code object of path."""
    out = {}
    for co in code_objects(path, work, tag):
        if os.path.getsize(co) == 0:
            continue
        funcs, kds = {}, {}
        for line in tool("llvm-readelf", "-s", "--wide", co, text=True).splitlines():
            p = line.split()
            if len(p) == 8 and p[3] == "FUNC" and p[6] != "UND":
                funcs[p[7]] = (int(p[1], 16), int(p[2]))
            elif len(p) == 8 and p[3] == "OBJECT" and p[7].endswith(".kd"):
                kds[p[7][:-3]] = (int(p[1], 16), int(p[2]))
        rodata = None
        for line in tool("llvm-readelf", "-S", "--wide", co, text=True).splitlines():
            m = re.match(r"\s*\[\s*\d+\]\s+\.rodata\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
            if m:
                rodata = tuple(int(x, 16) for x in m.groups())                     # address, file offset, size
        blob = open(co, "rb").read()
        body, cur, end = {}, None, 0
        for line in tool("llvm-objdump", "-d", co, text=True).splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                cur = m.group(1) if m.group(1) in funcs else None
                if cur:
                    body[cur], end = [], funcs[cur][0] + funcs[cur][1]
                continue
            m = re.match(r"^(.*?)//\s*([0-9A-Fa-f]+):", line)
            if cur and m and m.group(1).strip() and int(m.group(2), 16) < end:
                body[cur].append(m.group(1).strip())
        for name, (addr, size) in kds.items():
            if name in out:
                sys.exit("kernel defined twice in " + path + ": " + name)
            desc = blob[rodata[1] + addr - rodata[0]:][:size] if rodata and rodata[0] <= addr < rodata[0] + rodata[2] else b""
            if len(desc) != 64 or not body.get(name):                              # "identical" must never mean "nothing was compared"
                sys.exit("no descriptor or no instructions found for kernel " + name + " in " + path)
            out[name] = (body[name], desc[:16] + desc[24:])               # bytes 16..23: the code's offset from the descriptor
    return out


def plain_names(ks, namespaces, path):
    """ks keyed by demangled name without the given namespace qualifiers (and never with `(anonymous namespace)::`)."""
    names = sorted(ks)
    cxxfilt = os.path.join(LLVM, "llvm-cxxfilt")
    plain = subprocess.check_output([cxxfilt if os.path.exists(cxxfilt) else "c++filt"], input="\n".join(names), text=True).splitlines()
    if len(plain) != len(names):
        sys.exit("c++filt returned %d names for %d symbols of %s" % (len(plain), len(names), path))
    strip = re.compile(r"\(anonymous namespace\)::|" + "|".join(r"\b%s::" % re.escape(ns) for ns in namespaces))
    out = {}
    for sym, name in zip(names, plain):
        name = strip.sub("", name)
        if name in out:
            sys.exit("two kernels of " + path + " are both `" + name + "` once the namespaces are stripped (the second: " + sym + ")")
        out[name] = ks[sym]
    return out


def renamed(ks, path):
    """ks (the old side, by plain name) under the map in the file at path: lines of `old name<TAB>new name`."""
    table = {}
    for n, line in enumerate(open(path).read().splitlines(), 1):
        if not line.strip() or line.startswith("#"):
            continue
        pair = line.split("\t")
        if len(pair) != 2 or not pair[0] or not pair[1] or pair[0] in table:
            sys.exit("%s:%d: want `old name<TAB>new name`, each old name once" % (path, n))
        if pair[0] not in ks:
            sys.exit("%s:%d: no kernel of the old build is `%s`" % (path, n, pair[0]))
        table[pair[0]] = pair[1]
    out = {}
    for name, v in ks.items():
        to = table.get(name, name)
        if to in out:
            sys.exit("%s: two kernels of the old build end on the name `%s`" % (path, to))
        out[to] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old", help="build directory (csrc/build) or libazk.so of the build to compare against")
    ap.add_argument("new", help="the same of the build under test")
    ap.add_argument("--match", default="", help="compare only the kernels whose name (mangled; demangled under --strip-namespace) contains this")
    ap.add_argument("--quiet", action="store_true", help="print only the kernels that differ and the summary line")
    ap.add_argument("--strip-namespace", action="append", default=[], metavar="NS",
                    help="compare by demangled name less the qualifiers NS:: and (anonymous namespace):: (repeatable)")
    ap.add_argument("--rename", metavar="FILE", help="lines of `old demangled name<TAB>new demangled name`, applied to the old side before "
                    "pairing (needs --strip-namespace)")
    a = ap.parse_args()
    if "" in a.strip_namespace:
        ap.error("--strip-namespace needs a name")
    if a.rename and not a.strip_namespace:
        ap.error("--rename maps demangled names: it needs --strip-namespace")
    with tempfile.TemporaryDirectory() as work:
        old, new = kernels(a.old, work, "old"), kernels(a.new, work, "new")
    if a.strip_namespace:
        old, new = plain_names(old, a.strip_namespace, a.old), plain_names(new, a.strip_namespace, a.new)
    if a.rename:
        old = renamed(old, a.rename)
    old = {k: v for k, v in old.items() if a.match in k}
    new = {k: v for k, v in new.items() if a.match in k}
    if not old:
        print("no kernel matches", a.match)
        return 1
    differ, missing = [], []
    for k in sorted(old):
        if k not in new:
            missing.append(k)
            print("MISSING", k)
            continue
        what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if old[k][i] != new[k][i]]
        if what:
            differ.append(k)
        if what or not a.quiet:
            count = "%d -> %d" % (len(old[k][0]), len(new[k][0])) if what else "%d" % len(old[k][0])
            print("DIFFERENT (%s)" % ", ".join(what) if what else "same", count, "instructions", k)
    added = sorted(k for k in new if k not in old)
    for k in added:
        print("NEW", k)
    print("%d kernels in the old build: %d identical, %d different, %d missing; %d only in the new build"
          % (len(old), len(old) - len(differ) - len(missing), len(differ), len(missing), len(added)))
    return 1 if differ or missing or added else 0


if __name__ == "__main__":
    sys.exit(main())
