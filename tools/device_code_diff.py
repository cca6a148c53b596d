#!/usr/bin/env python3
"""
Compares the gfx950 device code of this tree with that of another tree (a `git worktree` of the parent commit, say): a host-side refactor is
harmless when every object holds the same kernels with the same instructions.
    python tools/device_code_diff.py OTHER_TREE [--keep DIR]
Both trees are built with their own phiflow_amd/csrc/Makefile into separate BUILD= / OUT= directories (a temporary directory, or DIR). Per object
file: the symbols only one tree has, the symbols whose size (or absolute value) differs, and whether the disassembly text is equal. `__hip_cuid_*` (a hash of the
source text) is ignored. Exit status 1 on any other difference.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
IGNORED = re.compile(r"__hip_cuid_")


def run(*cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def build(tree, out):
    csrc = os.path.join(tree, "phiflow_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j16", "ARCH=gfx950", f"BUILD={out}", f"OUT={os.path.join(out, 'libphihip.so')}"], check=True,
                   stdout=subprocess.DEVNULL)


def device_code(obj):
    """(symbol -> (size, value of an absolute symbol), disassembly without the ignored symbols' lines) of the gfx950 code object inside a host object file"""
    if ".hip_fatbin" not in run(os.path.join(LLVM, "llvm-objdump"), "-h", obj):
        return {}, ""                 # an object without kernels (capi.o)
    fat, co = obj + ".hipfb", obj + ".gfx950.co"
    run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    symbols = {}
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-t", co).splitlines():
        m = re.match(r"([0-9a-f]{16}) .{7} (\S+)\s+([0-9a-f]{16})\s+(?:\.\w+\s+)?(\S+)$", line)     # value flags section size [visibility] name
        if m and m.group(2) != "*UND*" and not IGNORED.search(m.group(4)):
            # (an absolute symbol -- a kernel's register counts, its scratch size -- carries its figure as the value, not as an address)
            symbols[m.group(4)] = (int(m.group(3), 16), m.group(1) if m.group(2) == "*ABS*" else None)
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    lines = [l for l in text.splitlines() if not IGNORED.search(l) and "file format" not in l and not l.endswith(".co:")]
    return symbols, "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other_tree")
    ap.add_argument("--keep", help="build into DIR/this and DIR/other and leave them there (default: a temporary directory)")
    args = ap.parse_args()
    other = os.path.abspath(args.other_tree)
    tmp = None if args.keep else tempfile.TemporaryDirectory(prefix="device_code_diff_")
    base = os.path.abspath(args.keep) if args.keep else tmp.name
    dirs = {"this": os.path.join(base, "this"), "other": os.path.join(base, "other")}
    build(ROOT, dirs["this"])
    build(other, dirs["other"])
    objs = {k: sorted(f for f in os.listdir(d) if f.endswith(".o")) for k, d in dirs.items()}
    differences = 0
    if objs["this"] != objs["other"]:
        print(f"object files differ: this {objs['this']} other {objs['other']}")
        differences += 1
    for name in sorted(set(objs["this"]) & set(objs["other"])):
        (sym_a, dis_a), (sym_b, dis_b) = (device_code(os.path.join(dirs[k], name)) for k in ("this", "other"))
        only_a, only_b = sorted(set(sym_a) - set(sym_b)), sorted(set(sym_b) - set(sym_a))
        resized = sorted(s for s in set(sym_a) & set(sym_b) if sym_a[s] != sym_b[s])
        same_text = dis_a == dis_b
        ok = not only_a and not only_b and not resized and same_text
        differences += 0 if ok else 1
        print(f"{name:18s} {len(sym_a):5d} symbols  only here {len(only_a)}  only there {len(only_b)}  size differs {len(resized)}  "
              f"disassembly {'equal' if same_text else 'DIFFERS'} ({len(dis_a.splitlines())} lines)")
        for label, group in (("only here", only_a), ("only there", only_b), ("size differs", resized)):
            for s in group[:20]:
                print(f"    {label}: {s}")
    print(f"{len(objs['this'])} objects, {differences} with differences")
    return 1 if differences else 0


if __name__ == "__main__":
    sys.exit(main())
