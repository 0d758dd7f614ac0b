#!/usr/bin/env python3
"""The device code of build/isa/ against the assembly of another build (the commit before), instruction by instruction:

    python profiles/explain_own/isa_compare.py <other isa dir>

profiles/kernel_manifest.py --diff compares a kernel's text whole, comments included, and the compiler's comments name IR blocks by a
running number (`; %Flow8184`, `; %.lr.ph4796`) that moves whenever ANY template of the unit gains a block -- so a change confined to one
instantiation of simon_wide.hip marks every kernel of the three units that include it.  Here a kernel is its instructions, directives and
.amdhsa_ / metadata entries with the comments cut off: equal text = equal code object bytes.  For the kernels that do differ the register,
LDS and scratch figures of both builds are listed."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kernel_manifest as km  # noqa: E402

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def code(body):
    return [ln for ln in (re.sub(r"\s*;.*$", "", x) for x in body.split("\n")) if ln.strip()]


def figures(body):
    return {f: int(m.group(1)) for f in FIELDS for m in [re.search(r"^\s+%s:\s+(\d+)" % re.escape(f), body, re.M)] if m}


def main(other):
    bad = 0
    for unit in sorted(km.scan()):
        a, b = km.bodies(os.path.join(km.ISA, unit + ".s")), km.bodies(os.path.join(other, unit + ".s"))
        moved = [k for k in sorted(a) if k not in b or code(a[k]) != code(b[k])]
        print(f"{unit}: {len(a)} kernels, {len(moved)} differ in code or metadata" + ("" if set(a) == set(b) else "  (kernel sets differ)"))
        for k in moved:
            fa, fb = figures(a[k]), figures(b.get(k, ""))
            print(f"  {k}\n    instructions+directives {len(code(b.get(k, '')))} -> {len(code(a[k]))}")
            print("    " + ", ".join(f"{f[1:]} {fb.get(f)} -> {fa.get(f)}" for f in FIELDS))
        bad += len(moved) if unit != "simon_wide_explain" else 0
    return bad


if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1]) else 0)
