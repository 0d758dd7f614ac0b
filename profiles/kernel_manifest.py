#!/usr/bin/env python3
"""The kernels of every translation unit, by mangled name, from the gfx950 assembly build() leaves in build/isa/<unit>.s.

  python profiles/kernel_manifest.py            writes profiles/kernel_manifest.txt from build/isa/
  python profiles/kernel_manifest.py --check    compares build/isa/ with the committed manifest (what tests/test_host.py does)
  python profiles/kernel_manifest.py --diff DIR compares build/isa/ with the assembly of another build, kernel by kernel

The manifest pins the set of instantiations: a dispatcher that names one template combination too many (build time, code size) or
one too few (a launch refused for inputs only a fuzzer reaches) changes it.  --diff is the check of a host-side refactor: the code and
the .amdhsa_ metadata of every kernel must not move.  Local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...) are numbered by a function's
position in the file (and named again in the loop comments), so they are normalised; the order of the kernels in the file is not compared."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "build", "isa")
MANIFEST = os.path.join(ROOT, "profiles", "kernel_manifest.txt")


def kernels(path):
    """sorted mangled names of the kernels of one assembly file"""
    return sorted(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path).read(), re.M))


def scan(isa_dir=ISA):
    """{unit: [names]} of every <unit>.s in isa_dir"""
    return {os.path.basename(p)[:-2]: kernels(p) for p in sorted(glob.glob(os.path.join(isa_dir, "*.s")))}


def read_manifest(path=MANIFEST):
    units, cur = {}, None
    for line in open(path).read().split("\n"):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        if line.startswith("["):
            cur = units.setdefault(line[1:line.index("]")], [])
        else:
            cur.append(line)
    return units


def write_manifest(units, path=MANIFEST):
    with open(path, "w") as f:
        f.write("# Kernels per translation unit (sorted mangled names), written by profiles/kernel_manifest.py from build/isa/*.s.\n")
        f.write(f"# {sum(len(v) for v in units.values())} kernels in {len(units)} units.\n")
        for unit, names in units.items():
            f.write(f"\n[{unit}] {len(names)}\n" + "".join(n + "\n" for n in names))


def compare(have, want):
    """differences between two {unit: [names]}: (unit, missing names, unexpected names) for every unit that differs"""
    out = []
    for unit in sorted(set(have) | set(want)):
        h, w = set(have.get(unit, [])), set(want.get(unit, []))
        if h != w:
            out.append((unit, sorted(w - h), sorted(h - w)))
    return out


def bodies(path):
    """{kernel: its code and .amdhsa_ block (label to the end of its `Kernel info` comment) + its entry of amdhsa.kernels}, local labels normalised"""
    text = open(path).read()
    meta = {}
    block = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.target:", text, re.M | re.S)
    for entry in re.split(r"^  - ", block.group(1) if block else "", flags=re.M)[1:]:
        meta[re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)] = entry
    out = {}
    for name in kernels(path):
        m = re.search(r"^%s:.*?\.section\t\.AMDGPU\.csdata.*?\n(?=\t\.)" % re.escape(name), text, re.M | re.S)
        body = re.sub(r"(\.L[A-Za-z_]+|\bBB)\d+", r"\1N", m.group(0))
        out[name] = re.sub(r"[ \t]+;", " ;", body) + meta[name]   # (a comment's column moves with the width of its label)
    return out


def diff(other_dir, isa_dir=ISA):
    bad = 0
    mine, theirs = scan(isa_dir), scan(other_dir)
    for unit, missing, extra in compare(mine, theirs):
        bad += 1
        print(f"{unit}: {len(missing)} kernels missing, {len(extra)} unexpected")
    for unit in sorted(set(mine) & set(theirs)):
        a, b = os.path.join(isa_dir, unit + ".s"), os.path.join(other_dir, unit + ".s")
        cuid = lambda p: re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", open(p).read())   # (the unit's id: a hash over its source)
        if cuid(a) == cuid(b):
            print(f"{unit}: {len(mine[unit])} kernels, files identical")
            continue
        ba, bb = bodies(a), bodies(b)
        moved = [k for k in ba if k in bb and ba[k] != bb[k]]
        bad += len(moved)
        print(f"{unit}: {len(mine[unit])} kernels, order differs, {len(moved)} kernels differ" + "".join("\n  " + k for k in moved))
    return bad


if __name__ == "__main__":
    if "--diff" in sys.argv:
        sys.exit(1 if diff(sys.argv[sys.argv.index("--diff") + 1]) else 0)
    if "--check" in sys.argv:
        d = compare(scan(), read_manifest())
        for unit, missing, extra in d:
            print(f"{unit}: missing {missing}, unexpected {extra}")
        sys.exit(1 if d else 0)
    write_manifest(scan())
