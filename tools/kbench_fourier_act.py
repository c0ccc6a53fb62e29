"""The FourierELU kernels alone, and the steerable.yaml network's eval forward with and without them: python tools/kbench_fourier_act.py

1. eqa_fourier_elu_fwd / _bwd on a (256, 144, 90, 90) channels-last map (1.19 GB: beyond the 256 MB last-level cache) against
   torch's clone() of the same map, alternating, back to back.  frac_of_copy = time of clone() moving the same bytes / kernel time
   (forward: one map read, one written = one clone; backward: two read, one written = 1.5 clones).
2. ESCNNSteerableNetwork((3, 96, 96), 16 fields, k = 7, 3 layers) eval forward at B = 256: the device path (norm folded into the
   kernel) against the same network with the op-by-op activation (EQA_FOURIER_KERNEL=0), alternating.
One JSON line per measurement.  --small: toy sizes, to rehearse the script."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import equiadapt_amd as ea
from equiadapt_amd import ops

dev = torch.device("cuda:0")
small = "--small" in sys.argv


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, n, rounds):
    """Each fn timed `rounds` times over n back-to-back calls, alternating; returns the median per fn and the spread."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, n))
    return {k: sorted(v)[len(v) // 2] for k, v in got.items()}, {k: (min(v), max(v)) for k, v in got.items()}


shape = (4, 144, 30, 30) if small else (256, 144, 90, 90)
x = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)
dy = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)
scale, shift = torch.rand(16, 5, device=dev) + 0.5, torch.rand(16, device=dev)
med, spread = alternate({"clone": lambda: x.clone(), "fwd": lambda: ops.fourier_elu(x, scale, shift), "fwd_plain": lambda: ops.fourier_elu(x),
                         "bwd": lambda: ops.fourier_elu_bwd(x, dy)}, n=20, rounds=5)
gb = x.numel() * 4 / 1e9
print(json.dumps({"what": "fourier_elu kernels", "shape": list(shape), "map_GB": round(gb, 3),
                  "clone_ms": med["clone"], "fwd_scale_shift_ms": med["fwd"], "fwd_ms": med["fwd_plain"], "bwd_ms": med["bwd"],
                  "fwd_frac_of_copy": med["clone"] / med["fwd"], "bwd_frac_of_copy": 1.5 * med["clone"] / med["bwd"],
                  "clone_TBps": 2 * gb / med["clone"], "fwd_TBps": 2 * gb / med["fwd"], "bwd_TBps": 3 * gb / med["bwd"],
                  "min_max_ms": spread}))
del x, dy
torch.cuda.empty_cache()

B, hw = (4, 48) if small else (256, 96)
torch.manual_seed(0)
net = ea.ESCNNSteerableNetwork((3, hw, hw), 16, 7, "rotation", 3).to(dev).eval()
img = torch.randn(B, 3, hw, hw, device=dev)


def run(kernel):
    os.environ["EQA_FOURIER_KERNEL"] = "1" if kernel else "0"
    with torch.no_grad():
        return net(img)


ref, got = run(False), run(True)
err = float((got - ref).abs().max() / ref.abs().max())
med, spread = alternate({"kernel": lambda: run(True), "plain": lambda: run(False)}, n=3, rounds=3)
os.environ["EQA_FOURIER_KERNEL"] = "1"
with ops.KernelTimer() as t:
    run(True)
print(json.dumps({"what": "steerable.yaml network eval forward", "B": B, "hw": hw, "kernel_activation_ms": med["kernel"],
                  "plain_op_activation_ms": med["plain"], "speedup": med["plain"] / med["kernel"], "rel_diff_of_outputs": err,
                  "min_max_ms": spread, "library_kernels_ms": {k: v[1] for k, v in t.summary().items()}}))
