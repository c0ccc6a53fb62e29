"""The field-norm training kernels alone, and the steerable.yaml network's training step with and without them:
python tools/kbench_field_norm.py [--small] [--step-only]

1. eqa_field_norm_stats / _elu_bwd_reduce / _elu_bwd_apply on a (256, 144, 90, 90) channels-last map (1.19 GB: beyond the 256 MB
   last-level cache) against torch's clone() of the same map, alternating, back to back; eqa_fourier_elu_bwd beside them as the
   sibling of the apply pass.  frac_of_copy = time of clone() moving the same bytes / kernel time (statistics: one map read = 0.5
   clone; reduce: two read = 1 clone; apply: two read, one written = 1.5 clones).
2. ESCNNSteerableNetwork((3, 96, 96), 16 fields, k = 7, 3 layers) training step at B = 256, forward + backward of (out * w).sum():
   EQA_FIELD_NORM_KERNEL=1 against 0, alternating, with torch.cuda.max_memory_allocated of each and the library's launches of one
   step.  Only the public class and the knob are used, so the script also runs on a commit that does not know the knob (both
   columns are then the same route): the comparison between commits is this part in fresh processes (--step-only), A-B-A.
One JSON line per measurement, medians of 5 x 20 (kernels) / 5 x 3 (steps) with the (min, max) of the rounds.  --small: toy sizes,
to rehearse the script."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import equiadapt_amd as ea
from equiadapt_amd import ops

dev = torch.device("cuda:0")
small = "--small" in sys.argv
KNOB = "EQA_FIELD_NORM_KERNEL"


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


if "--step-only" not in sys.argv:
    shape = (4, 144, 30, 30) if small else (256, 144, 90, 90)
    x = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)
    scale, shift, coef = torch.rand(16, 5, device=dev) + 0.5, torch.rand(16, device=dev), 0.01 * torch.rand(16, 7, device=dev)
    med, spread = alternate({"clone": lambda: x.clone(), "stats": lambda: ops.field_norm_stats(x),
                             "reduce": lambda: ops.field_norm_elu_bwd_reduce(x, dy, scale, shift),
                             "apply": lambda: ops.field_norm_elu_bwd_apply(x, dy, scale, shift, coef),
                             "elu_bwd": lambda: ops.fourier_elu_bwd(x, dy, scale, shift)}, n=20, rounds=5)
    gb = x.numel() * 4 / 1e9
    print(json.dumps({"what": "field_norm kernels", "shape": list(shape), "map_GB": round(gb, 3),
                      "partial_rows": ops.field_norm_stats(x).shape[0], "clone_ms": med["clone"], "stats_ms": med["stats"],
                      "bwd_reduce_ms": med["reduce"], "bwd_apply_ms": med["apply"], "fourier_elu_bwd_ms": med["elu_bwd"],
                      "stats_frac_of_copy": 0.5 * med["clone"] / med["stats"], "bwd_reduce_frac_of_copy": med["clone"] / med["reduce"],
                      "bwd_apply_frac_of_copy": 1.5 * med["clone"] / med["apply"],
                      "fourier_elu_bwd_frac_of_copy": 1.5 * med["clone"] / med["elu_bwd"],
                      "clone_TBps": 2 * gb / med["clone"], "stats_TBps": gb / med["stats"], "bwd_reduce_TBps": 2 * gb / med["reduce"],
                      "bwd_apply_TBps": 3 * gb / med["apply"], "min_max_ms": spread}), flush=True)
    del x, dy
    torch.cuda.empty_cache()

B, hw = (4, 48) if small else (256, 96)
torch.manual_seed(0)
net = ea.ESCNNSteerableNetwork((3, hw, hw), 16, 7, "rotation", 3).to(dev).train()
img = torch.randn(B, 3, hw, hw, device=dev)
w = torch.randn(B, 2, 2, device=dev)


def step(knob):
    os.environ[KNOB] = knob
    net.zero_grad(set_to_none=True)
    out = net(img)
    (out * w).sum().backward()
    return out.detach()


def peak(knob):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    step(knob)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


ref, got = step("0"), step("1")
err = float((got - ref).abs().max() / ref.abs().max())
grads = {k: p.grad.clone() for k, p in net.named_parameters()}
step("0")
gerr = max(float((p.grad - grads[k]).abs().max() / grads[k].abs().max().clamp_min(1e-30)) for k, p in net.named_parameters())
med, spread = alternate({"knob_1": lambda: step("1"), "knob_0": lambda: step("0")}, n=3, rounds=5)
mem = {"knob_1": peak("1"), "knob_0": peak("0")}
launches = {}
for knob in ("1", "0"):
    with ops.KernelTimer() as t:
        step(knob)
    launches["knob_" + knob] = {k: [v[0], round(v[1], 4)] for k, v in t.summary().items()}
os.environ[KNOB] = "1"
print(json.dumps({"what": "steerable.yaml network training step", "B": B, "hw": hw, "knob_1_ms": med["knob_1"], "knob_0_ms": med["knob_0"],
                  "speedup": med["knob_0"] / med["knob_1"], "peak_MiB": mem, "rel_diff_of_outputs": err, "rel_diff_of_gradients": gerr,
                  "min_max_ms": spread, "library_launches_count_mean_ms": launches}), flush=True)
