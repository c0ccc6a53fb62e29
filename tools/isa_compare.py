#!/usr/bin/env python
"""Compare two builds of a translation unit kernel by kernel (the evidence of a refactor that must not change the generated code).

  hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -std=c++17 -Iinclude --cuda-device-only -S csrc/UNIT.hip -o UNIT.s
  python tools/isa_compare.py PARENT.s[,PARENT2.s] BRANCH.s[,BRANCH2.s]     (several files: a unit that was split)

Per kernel symbol, comments and assembler directives are stripped and basic-block labels renumbered per kernel (the function index
in `.LBBn_m` depends on the unit).  Prints one markdown table row per kernel: instruction counts, and for a kernel that differs
the index of the first differing instruction and the number of differing positions."""
import re
import subprocess
import sys


def kernels(paths):
    out = {}
    for path in paths.split(","):
        cur = None
        for line in open(path):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = m.group(1)
                out[cur] = []
                continue
            if cur is None:
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            t = line.split(";")[0].rstrip()
            if not t.strip() or re.match(r"^\s+\.", t):
                continue
            out[cur].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t).strip())
    return out


def demangle(name):
    res = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return res.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = 0
    print("| kernel | instructions, parent | branch | |\n|---|---|---|---|")
    for k in sorted(set(a) | set(b), key=demangle):
        if k not in a or k not in b:
            print(f"| `{demangle(k)}` | | | only in the {'parent' if k in a else 'branch'} |")
            continue
        ia = [x for x in a[k] if not x.endswith(":")]
        ib = [x for x in b[k] if not x.endswith(":")]
        if a[k] == b[k]:
            same += 1
            print(f"| `{demangle(k)}` | {len(ia)} | {len(ib)} | identical |")
            continue
        first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
        nd = sum(1 for x, y in zip(ia, ib) if x != y) + abs(len(ia) - len(ib))
        print(f"| `{demangle(k)}` | {len(ia)} | {len(ib)} | first difference at {first}, {nd} positions differ |")
    print(f"\n{same} of {len(set(a) | set(b))} kernels identical instruction for instruction")


if __name__ == "__main__":
    main()
