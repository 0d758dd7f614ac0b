#!/usr/bin/env python3
"""The plain pod's path through the scheduling cycle of a straight-line score-table kernel, read off the emitted assembly: per body of the
kernel (a fused kernel holds two), the instructions from the loop header of the inner (64-step) loop to the branch back to the latch, plus the
latch block, counted by class as docs/KERNELS.md tabulates them since round 9.  The latch is found by its `v_writelane_b32 ..., m0` (the step
record); the rare blocks lie outside the range, and every region inside it is one the plain pod executes.
usage: python profiles/cycle_path.py build/isa/simon_table.s [kernel-name-substring] [--dump]
default kernel: config 3's fused one, table_kernel<true, true, false, 1, 2, false, ..., LO = 1>."""
import re
import sys

C3 = "_ZN5simon12table_kernelILb1ELb1ELb0ELi1ELi2ELb0ELb0ELb0ELb0ELb0ELb0ELi1ELb0ELb0ELb0ELi1EEE"


def classes(lines):
    c = dict(v=0, s=0, branch=0, nop=0, wait=0, ds=0, mem=0)
    for ln in lines:
        op = ln.split()[0]
        if op == "s_nop":
            c["nop"] += 1
        elif op == "s_waitcnt":
            c["wait"] += 1
        elif op.startswith("s_"):
            c["s"] += 1
            c["branch"] += op.startswith(("s_cbranch", "s_branch"))
        elif op.startswith("v_"):
            c["v"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["mem"] += 1
    c["issued"] = c["v"] + c["s"] + c["nop"] + c["wait"] + c["ds"] + c["mem"]
    return c


def bodies(path, name):
    text = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(text) if ln.startswith(name) and ln.rstrip().split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
    fn = text[start:end]
    is_label = lambda ln: re.match(r"^\.LBB\d+_\d+:", ln)                      # noqa: E731
    is_code = lambda ln: ln.startswith("\t") and not ln.strip().startswith((";", "."))   # noqa: E731
    out = []
    for i, ln in enumerate(fn):
        if not re.search(r"v_writelane_b32 v\d+, s\d+, m0", ln):
            continue
        a = max(j for j in range(i) if is_label(fn[j]))                       # the latch block's label
        latch = fn[a].split(":")[0]
        h = next(j for j in range(i, len(fn)) if is_label(fn[j]))             # the loop header
        e = next(j for j in range(h, len(fn)) if re.search(r"s_c?branch\w*\s+" + re.escape(latch) + r"\b", fn[j]) and "wave barrier" in " ".join(fn[j - 3:j]))
        out.append([x.strip() for x in fn[a:h] + fn[h:e + 1] if is_code(x)])
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = args[1] if len(args) > 1 else C3
    for n, body in enumerate(bodies(args[0], name)):
        c = classes(body)
        print(f"body {n}: v_ {c['v']}  s_ {c['s']} (branches {c['branch']})  s_nop {c['nop']}  s_waitcnt {c['wait']}  ds_ {c['ds']}  global_ {c['mem']}  issued {c['issued']}")
        if "--dump" in sys.argv:
            print("\n".join("    " + x for x in body))


if __name__ == "__main__":
    main()
