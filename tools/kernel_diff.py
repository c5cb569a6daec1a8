#!/usr/bin/env python3
"""Compare the gfx950 device code of two build trees, symbol by symbol.

    python tools/kernel_diff.py PARENT_TREE THIS_TREE [--only conv,gemm256] [--keep DIR] [-j N] [-q]

Route: per-file assembly.  For each tree, every `*.hip` of its `r-yolov4_amd/csrc` is compiled with that tree's own Makefile flags
(`COMMON` and `FLAGS_<file>`) plus `--cuda-device-only -S`; nothing is unbundled from a built library.  A tree argument may be the repository
root, its csrc directory, or a directory of `<file>.s` written by an earlier run with --keep (so the parent is compiled once).

The assembly of a file is cut into chunks, one per symbol: a function or object from its `.type` line or label to the next one, a kernel
descriptor from `.amdhsa_kernel NAME` to `.end_amdhsa_kernel` (VGPR / SGPR / AGPR counts, LDS, scratch, kernarg size, ...), and the file's
metadata note.  Comments and blank lines are dropped, the compiler's local labels (`.LBB12_3`, `.Lfunc_end12`) lose their per-file function
number and the `__hip_cuid_<hash>` marker object (a hash of the file's path) loses its hash; everything else, every instruction with its
registers and every descriptor field, is compared as plain text.  Per symbol the report says `identical` or shows the first differing line; a
symbol on one side only is a difference.  Exit status 1 when anything differs.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")
SYMBOL = re.compile(r"^(?:([A-Za-z_$][\w$.]*):|\s+\.type\s+([A-Za-z_$][\w$.]*),)")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")          # hipcc's per-compilation id symbol: a hash of the file's path and options, no device code


def csrc_of(tree):
    for d in (tree, os.path.join(tree, "r-yolov4_amd", "csrc")):
        if os.path.exists(os.path.join(d, "Makefile")) or any(f.endswith(".s") for f in os.listdir(d)):
            return d
    sys.exit(f"{tree}: neither a build tree nor a directory of .s files")


def make_flags(csrc):
    """COMMON and FLAGS_<file> of the tree's Makefile, $(ARCH) expanded."""
    v = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M))
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: v.get(m.group(1), ""), s)
    return expand(v["COMMON"]).split(), {k[6:]: expand(s).split() for k, s in v.items() if k.startswith("FLAGS_")}


def assembly(tree, only, keep, jobs):
    """{file stem: assembly text} of one tree."""
    csrc = csrc_of(tree)
    stems = sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".hip"))
    if not stems:                                                   # a directory kept by an earlier run
        return {f[:-2]: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".s") and (not only or f[:-2] in only)}
    common, per_file = make_flags(csrc)
    out = keep or tempfile.mkdtemp(prefix="kernel_diff_")
    os.makedirs(out, exist_ok=True)

    def one(stem):
        s = os.path.join(out, stem + ".s")
        subprocess.run([HIPCC, *common, *per_file.get(stem, []), "--cuda-device-only", "-S", "-Wno-unused-command-line-argument", stem + ".hip", "-o", s],
                       cwd=csrc, check=True)
        return stem, open(s).read()

    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        return dict(pool.map(one, [s for s in stems if not only or s in only]))


def chunks(text):
    """{symbol: [normalised lines]} of one file's assembly."""
    out, key = {}, "<header>"
    for line in text.splitlines():
        line = CUID.sub("__hip_cuid", LOCAL_LABEL.sub(r".L\1\2", line.split(";")[0].rstrip())) if '"' not in line else line.rstrip()
        if not line.strip():
            continue
        m = SYMBOL.match(line)
        if m:
            key = m.group(1) or m.group(2)
        elif line.lstrip().startswith(".amdhsa_kernel "):
            key = line.split()[1] + " [descriptor]"
        elif line.lstrip().startswith(".amdgpu_metadata"):
            key = "<metadata>"
        out.setdefault(key, []).append(line)
        if line.lstrip().startswith(".end_amdhsa_kernel"):
            key = "<between>"
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="parent: repository root, csrc directory, or directory of kept .s files")
    ap.add_argument("b", help="the tree under test, same forms")
    ap.add_argument("--only", default="", help="comma-separated file stems (default: every .hip)")
    ap.add_argument("--keep", default="", help="write the assembly to DIR/a and DIR/b and keep it")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="parallel compiles")
    ap.add_argument("-q", action="store_true", help="print only differing symbols and the totals")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    asm = [assembly(t, only, args.keep and os.path.join(args.keep, side), args.j) for t, side in ((args.a, "a"), (args.b, "b"))]
    total = differing = kernels = 0
    for stem in sorted(set(asm[0]) | set(asm[1])):
        ca, cb = (chunks(x.get(stem, "")) for x in asm)
        for sym in sorted(set(ca) | set(cb)):
            total += 1
            kernels += sym.endswith(" [descriptor]")
            la, lb = ca.get(sym), cb.get(sym)
            if la == lb:
                if not args.q:
                    print(f"{stem}: {sym}: identical ({len(la)} lines)")
                continue
            differing += 1
            if la is None or lb is None:
                print(f"{stem}: {sym}: only in {'b' if la is None else 'a'}")
                continue
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"{stem}: {sym}: DIFFERS at line {i + 1} of {len(la)} / {len(lb)}\n    a: {la[i] if i < len(la) else '<end>'}\n    b: {lb[i] if i < len(lb) else '<end>'}")
    print(f"{len(set(asm[0]) | set(asm[1]))} files, {total} symbols ({kernels} kernels), {differing} differing")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
