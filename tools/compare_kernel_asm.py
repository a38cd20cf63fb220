#!/usr/bin/env python3
"""Compares the kernels of two builds by the compiler's own assembly output (`make -C rust-tracer_amd/csrc asm` at two commits: the
product's rt_capi.gfx950.s or the hooks build's rt_capi_hooks.gfx950.s of each).

For every kernel of either file: whether its INSTRUCTION TEXT is the same in both -- comments stripped, directives dropped, the function
number in block labels (.LBB<n>_<k>) normalised, since it moves whenever a kernel is added or removed in front -- the instruction count of
each side, and the registers and scratch each side's metadata declares (.sgpr_count, .vgpr_count, .private_segment_fixed_size).  A
refactor that means to leave a kernel alone leaves its text alone; one that reshapes a kernel should keep its residency: no scratch, and
the same waves-per-SIMD class (vector registers rounded up to 8 go into 512; scalar registers <= 80 / <= 96 / above, as in
tests/test_kernel_resources.py).

usage: compare_kernel_asm.py OLD.s NEW.s [--may-differ REGEX] [--all]
  --may-differ REGEX   kernels whose demangled name matches are EXPECTED to differ: they are listed with their figures, and only a lost
                       residency class or scratch counts against them; every other kernel must be the same
  --all                list the identical kernels too (default: a count)
Exit status 1 when a kernel outside --may-differ differs, is missing on one side, or one inside it loses residency."""
import argparse
import re
import subprocess
import sys


def kernels_of(path):
    """{mangled name: (normalised instruction lines, resources dict)} of one .s file"""
    lines = open(path).read().split("\n")
    meta, cur = {}, None
    for l in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)):]:
        if re.match(r"^  - \.", l):
            cur = {}
        m = re.match(r"^  (?:- |  )\.(\w+):\s+(\S+)\s*$", l)       # (a kernel's own keys: its arguments' sit deeper)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    out = {}
    for first, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):\s*; @", l)
        if not m or m.group(1) not in meta:        # (device functions that are no kernels have no metadata entry)
            continue
        body = []
        for t in lines[first + 1:]:
            if t.startswith(".Lfunc_end"):
                break
            t = re.sub(r"\.LBB\d+_", ".LBB_", t.split(";", 1)[0].strip())
            if t and (not t.startswith(".") or t.endswith(":")):
                body.append(t)
        out[m.group(1)] = (body, meta[m.group(1)])
    return out


def residency(res):
    """(waves per SIMD by vector registers, scalar register class)"""
    v, s = int(res["vgpr_count"]) + int(res.get("agpr_count", 0)), int(res["sgpr_count"])
    return min(8, 512 // max(8, (v + 7) // 8 * 8)), (0 if s <= 80 else 1 if s <= 96 else 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--may-differ", default=None)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    old, new = kernels_of(a.old), kernels_of(a.new)
    names = sorted(set(old) | set(new))
    plain = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    same = bad = 0
    for n in names:
        short = re.sub(r"^void ", "", plain[n]).split("(")[0]
        if n not in old or n not in new:
            print("%-8s %s" % ("ONLY OLD" if n in old else "ONLY NEW", short))
            bad += 1
            continue
        (bo, ro), (bn, rn) = old[n], new[n]
        count = lambda b: sum(1 for t in b if not t.endswith(":"))
        fig = lambda r, b: "(%s, %s, %d)" % (r["sgpr_count"], r["vgpr_count"], count(b))
        expected = a.may_differ is not None and re.search(a.may_differ, plain[n]) is not None
        lost = int(rn["private_segment_fixed_size"]) != 0 or residency(rn) != residency(ro)
        if bo == bn and not expected:
            same += 1
            if a.all:
                print("same     %-90s %s" % (short, fig(rn, bn)))
            continue
        verdict = "same" if bo == bn else "differs"
        if not expected or lost:
            bad += 1
            verdict += " RESIDENCY LOST" if expected else " UNEXPECTED"
        print("%-8s %-90s old (sgpr, vgpr, instructions) %s new %s scratch %s -> %s" %
              (verdict, short, fig(ro, bo), fig(rn, bn), ro["private_segment_fixed_size"], rn["private_segment_fixed_size"]))
    print("%d kernels, %d outside --may-differ identical, %d problems" % (len(names), same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
