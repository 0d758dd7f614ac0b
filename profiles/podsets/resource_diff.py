#!/usr/bin/env python3
"""VGPR / SGPR / scratch / spill figures of every kernel, this build against another build's assembly, summarised per translation unit.
usage: python profiles/podsets/resource_diff.py OTHER_ISA_DIR [THIS_ISA_DIR=build/isa]      (directories of <unit>.s as build() leaves them)
A kernel is matched by its mangled name; the PODSETS = false instantiations of narrow_kernel / fast_kernel are matched with the other build's
kernel of the same remaining arguments.  Lists every kernel whose VGPR count crosses an occupancy step (waves per SIMD by VGPRs, 512 / granule 8)."""
import collections
import glob
import os
import re
import sys

KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def read(d):
    out = {}
    for f in glob.glob(os.path.join(d, "*.s")):
        for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)", open(f).read(), re.S):
            g = lambda k: re.search(r"\." + k + r":\s+(\S+)", m.group(0)).group(1)   # noqa: E731
            name = re.sub(r"((?:narrow|fast)_kernelI(?:L[ib]\d+E){4})Lb0E", r"\1", g("name"))
            out[(os.path.basename(f)[:-2], name)] = tuple(int(g(k)) for k in KEYS)
    return out


def occupancy(v):
    return min(8, 512 // (((v + 7) // 8) * 8))


def main():
    other, mine = read(sys.argv[1]), read(sys.argv[2] if len(sys.argv) > 2 else "build/isa")
    by = collections.defaultdict(list)
    for k, y in mine.items():
        if k in other:
            by[k[0]].append((k[1], other[k], y))
    print(f"kernels: other {len(other)}, this {len(mine)}, new here {len([k for k in mine if k not in other])}")
    print("unit | kernels | moved | dVGPR | dSGPR | dscratch B | dVGPR spills | dSGPR spills | VGPR occupancy steps crossed")
    for unit, lst in sorted(by.items()):
        moved = [(n, x, y) for n, x, y in lst if x != y]
        d = lambda i: f"{min((y[i] - x[i] for _, x, y in lst)):+d} .. {max((y[i] - x[i] for _, x, y in lst)):+d}"   # noqa: E731
        crossed = [(n, x[0], y[0]) for n, x, y in lst if occupancy(x[0]) != occupancy(y[0])]
        print(f"{unit} | {len(lst)} | {len(moved)} | {d(0)} | {d(1)} | {d(2)} | {d(3)} | {d(4)} | {len(crossed)}")
        for n, a, b in crossed:
            print(f"    {n}: {a} -> {b} VGPRs, {occupancy(a)} -> {occupancy(b)} waves per SIMD")


if __name__ == "__main__":
    main()
