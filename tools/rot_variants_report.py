#!/usr/bin/env python3
"""The record behind profiles/rot_variants.txt: which template instantiations of the rotated-lattice kernels the dispatcher can
choose (tests/rot_variants.py: the variant probe over its grid), how many the source compiles, and which ones a logged run of
the suite reached.  No GPU needed.

    tools/rot_variants_report.py [--code-objects DIR] [--log requests.jsonl]

--code-objects: a directory of device code objects (tools/device_code_diff.sh build <tree> DIR): kernels are counted per family
from their kernel descriptors' names.  --log: a request log of tools/request_log.py.
"""
import argparse
import collections
import ctypes
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rot_variants as rv      # noqa: E402

X_NAME = {"aai_quad_kernel": "-", "aai_quad_fast_kernel": "rows", "aai_quad_multi_kernel": "WORDS", "aai_cell_kernel": "WR",
          "aai_cell_multi_kernel": "WORDS", "aai_wide_kernel": "PARTS", "aai_wide_fast_kernel": "PARTS"}
# kernels of the code objects that belong to a family of the table (the fast family has two kernels: 16 x 4 and row-shaped waves)
KERNELS = {"aai_quad_kernel": ("aai_quad_kernel",), "aai_quad_fast_kernel": ("aai_quad_fast_kernel", "aai_quad_fast_rows_kernel"),
           "aai_quad_multi_kernel": ("aai_quad_multi_kernel",), "aai_cell_kernel": ("aai_cell_kernel",),
           "aai_cell_multi_kernel": ("aai_cell_multi_kernel",), "aai_wide_kernel": ("aai_wide_kernel",),
           "aai_wide_fast_kernel": ("aai_wide_fast_kernel",)}


def hostemu():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libaai_hostemu.so")
    src = os.path.join(ROOT, "tests", "emulation", "host_emulation.cpp")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    return ctypes.CDLL(so)


def compiled(directory):
    """family -> number of kernels in the code objects (the kernel descriptors <mangled name>.kd)"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    names = set()
    for co in sorted(glob.glob(os.path.join(directory, "*.co"))):
        for line in subprocess.run([readelf, "-sW", co], capture_output=True, text=True, check=True).stdout.splitlines():
            f = line.split()
            if len(f) >= 8 and f[7].endswith(".kd"):
                names.add(f[7][:-3])
    counts = collections.Counter()
    for fam, kernels in KERNELS.items():
        for k in kernels:
            tag = "%d%sI" % (len(k), k)              # Itanium mangling of a template-id: <length><name>I<arguments>E
            counts[fam] += sum(1 for n in names if tag in n)
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code-objects")
    ap.add_argument("--log")
    a = ap.parse_args()
    cands, cases, probe = rv.table(hostemu())
    print("grid: " + rv.GRID)
    print("candidates: %d; cases: %d (two per candidate)" % (len(cands), len(cases)))
    print()
    print("== candidates per family, plain images (C = 1); the 8- and 16-bit sources have the same set ==")
    plain = sorted(c for c in cands if c.T == "f32" and c.C == 1)
    for fam in KERNELS:
        mine = [c for c in plain if c.family == fam]
        if not mine:
            continue
        print("%s: %d   (WIN, SCALED, HP, %s)" % (fam, len(mine), X_NAME[fam]))
        print("    " + " ".join("(%d,%d,%d,%d)" % (c.win, c.scaled, c.hp, c.x) for c in mine))
    print("total: %d per source type" % len(plain))
    print()
    print("== interleaved candidates (area mode; fast mode with channels stays on the double-precision kernel) ==")
    for fam in ("aai_quad_multi_kernel", "aai_cell_multi_kernel"):
        for T in rv.TYPES:
            for C in (2, 3, 4):
                mine = sorted(c for c in cands if (c.family, c.T, c.C) == (fam, T, C))
                kept = [c for c in mine if not cands[c][2]]
                print("%s %s C=%d: %d candidates (WORDS %s), %d dispatched, not dispatched: WIN %s" % (
                    fam, T, C, len(mine), sorted({c.x for c in mine}), len(mine) - len(kept), sorted({c.win for c in kept}) or "-"))
    print()
    # distinct template arguments among the dispatched candidates: a candidate also keeps apart what one kernel branches on at run
    # time (HP in aai_quad_multi_kernel) and the channel counts that share a slot size (WORDS)
    def instantiation(c):
        return (c.family, c.T, c.win, c.scaled, c.x) if c.family == "aai_quad_multi_kernel" else (c.family, c.T, c.win, c.scaled, c.hp, c.x)
    per_family = collections.Counter(i[0] for i in {instantiation(c) for c in cands if cands[c][2]})
    if a.code_objects:
        counts = compiled(a.code_objects)
        print("== kernels the source compiles against instantiations the dispatcher can choose (all types and channel counts) ==")
        for fam in KERNELS:
            print("%-24s compiled %4d   dispatchable %4d" % (fam, counts[fam], per_family[fam]))
        print("%-24s compiled %4d   dispatchable %4d" % ("total", sum(counts.values()), sum(per_family.values())))
        print("(dispatchable: distinct template arguments among the dispatched candidates; the fast family's row-shaped wave is a kernel")
        print(" of its own and counts as one)")
        print()
    if a.log:
        reached = collections.defaultdict(set)
        calls = 0
        for line in open(a.log):
            r = json.loads(line)
            if r["rc"] != 0 or r["mode"] not in (rv.MODE_AREA, rv.MODE_FAST):
                continue
            calls += 1
            T = {0: "f32", 1: "u8", 2: "u16"}[r["dtype"]]
            where = dict(W=r["src_width"], H=r["src_height"], iso=(r["src_iso_x"], r["src_iso_y"]), dst_res=r["dst_res_x"])
            v = probe(r["src_res_x"], r["rotation_deg"], r["mode"], r["policy"], r["channels"], rv.TYPES[T][1], **where)
            fam = rv.FAMILIES.get(v.family)
            ran = r["kernel"].split("<")[0].split("+")[0]
            if fam not in KERNELS or ran != fam:
                continue
            one = [c for c, (policy, ok) in rv.hosted(probe, r["src_res_x"], r["rotation_deg"], r["mode"], T, r["channels"], **where).items()
                   if ok and c.family == fam]
            for c in one:
                reached[c.family].add(c)
        print("== candidates the suite reached before this module (%d logged area / fast calls; family that ran = candidate's family) ==" % calls)
        for T, C in [(T, 1) for T in rv.TYPES] + [("f32", 0), ("u8", 0), ("u16", 0)]:
            want = {c for c in cands if cands[c][2] and c.T == T and ((c.C == 1) if C == 1 else (c.C > 1))}
            got = {c for f in reached.values() for c in f} & want
            print("%s, %s: %d of %d" % (T, "C = 1" if C == 1 else "C > 1", len(got), len(want)))
            if C == 1:
                for fam in KERNELS:
                    miss = sorted(c for c in want - got if c.family == fam)
                    if miss:
                        print("    never reached, %s (WIN, SCALED, HP, %s): %s" % (fam, X_NAME[fam], " ".join("(%d,%d,%d,%d)" % (c.win, c.scaled, c.hp, c.x) for c in miss)))
        stray = {c for f in reached.values() for c in f} - set(cands)
        if stray:
            print("reached but not a candidate of the grid: %s" % sorted(stray))


if __name__ == "__main__":
    main()
