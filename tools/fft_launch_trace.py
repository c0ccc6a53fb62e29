#!/usr/bin/env python
"""Do two builds of libeqa_hip.so launch the same FFT kernels with the same grids and arguments?  Host code only, no GPU.

  python tools/fft_launch_trace.py PARENT.so BRANCH.so [OUT.txt]

Builds tools/micro/fft_launch_trace.cpp (g++), which drives every eqa_fft48k5_* / eqa_fft48_* entry point over maps, channel
counts, kernel sizes and options that reach every branch of the launch plan, and compares what the two libraries print under the
default environment, EQA_FFT_INV_PIPE=0 and EQA_FFT_TWO_PASS=1.  Writes a summary: launches per kernel and a digest per trace."""
import collections
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = [("default", {}), ("EQA_FFT_INV_PIPE=0", {"EQA_FFT_INV_PIPE": "0"}), ("EQA_FFT_TWO_PASS=1", {"EQA_FFT_TWO_PASS": "1"})]


def symbols(so, path):
    """offset, argument count and name of every kernel's host-side handle"""
    with open(path, "w") as f:
        for line in subprocess.run(["nm", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines():
            p = line.split()
            if len(p) != 3 or "kernel" not in p[2]:
                continue
            d = subprocess.run(["c++filt", p[2]], capture_output=True, text=True).stdout.strip()
            if "(" not in d:
                continue
            args = d[d.rindex("(") + 1:d.rindex(")")]
            name = d[:d.rindex("(")].replace("(anonymous namespace)::", "").replace("__device_stub__", "").replace("void ", "").replace(" ", "")
            f.write(f"{p[0]} {args.count(',') + 1 if args.strip() else 0} {name}\n")


def main():
    parent, branch = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else sys.stdout
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "fft_launch_trace")
    subprocess.run(["g++", "-O1", "-std=c++17", "-rdynamic", os.path.join(ROOT, "tools/micro/fft_launch_trace.cpp"), "-o", exe, "-ldl"], check=True)
    differ = 0
    for env_name, extra in ENVS:
        text = {}
        for label, so in (("parent", parent), ("branch", branch)):
            sym = os.path.join(tmp, label + ".sym")
            symbols(so, sym)
            text[label] = subprocess.run([exe, so, sym], capture_output=True, text=True, check=True, env=dict(os.environ, **extra)).stdout
        same = text["parent"] == text["branch"]
        differ += not same
        lines = text["branch"].splitlines()
        counts = collections.Counter(l.split("|")[1].split()[0] for l in lines if "|" in l)
        print(f"## {env_name}: {sum(1 for l in lines if '|' not in l)} cases, {sum(counts.values())} launches of {len(counts)} kernels; "
              f"sha256 parent {hashlib.sha256(text['parent'].encode()).hexdigest()[:16]} branch {hashlib.sha256(text['branch'].encode()).hexdigest()[:16]}"
              f" -- {'identical text' if same else 'DIFFERENT'}", file=out)
        for k in sorted(counts):
            print(f"{counts[k]:6d}  {k}", file=out)
        print(file=out)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
