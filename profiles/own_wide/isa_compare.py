#!/usr/bin/env python3
"""profiles/explain_own/isa_compare.py for a change that ADDS a translation unit: the units both builds have are compared kernel by
kernel (instructions, directives and metadata, comments cut off), a unit only this build has is listed with its kernels' figures.

    python profiles/own_wide/isa_compare.py <isa dir of the build before> > profiles/own_wide/isa_compare.txt"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "explain_own"))
import isa_compare as ic  # noqa: E402
from isa_compare import km  # noqa: E402


def main(other):
    bad = 0
    for unit in sorted(km.scan()):
        a = km.bodies(os.path.join(km.ISA, unit + ".s"))
        if not os.path.exists(os.path.join(other, unit + ".s")):
            print(f"{unit}: {len(a)} kernels, a new unit")
            for k in sorted(a):
                fa = ic.figures(a[k])
                print(f"  {k}\n    instructions+directives {len(ic.code(a[k]))}; " + ", ".join(f"{f[1:]} {fa.get(f)}" for f in ic.FIELDS))
            continue
        b = km.bodies(os.path.join(other, unit + ".s"))
        moved = [k for k in sorted(a) if k not in b or ic.code(a[k]) != ic.code(b[k])]
        print(f"{unit}: {len(a)} kernels, {len(moved)} differ in code or metadata" + ("" if set(a) == set(b) else "  (kernel sets differ)"))
        for k in moved:
            fa, fb = ic.figures(a[k]), ic.figures(b.get(k, ""))
            print(f"  {k}\n    instructions+directives {len(ic.code(b.get(k, '')))} -> {len(ic.code(a[k]))}")
            print("    " + ", ".join(f"{f[1:]} {fb.get(f)} -> {fa.get(f)}" for f in ic.FIELDS))
        bad += len(moved) + (set(a) != set(b))
    return bad


if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1]) else 0)
