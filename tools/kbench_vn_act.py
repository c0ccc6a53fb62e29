"""VNLeakyReLU / VNSoftplus on the device, fused route against plain route, same process, alternating: python tools/kbench_vn_act.py

Shapes: (32, 21, 3, 1024, 20), the first-block edge tensor of a VN-DGCNN, and (32, 85, 3, 1024, 1), its widest layer (256 // 3
channels).  Legs, each `rounds` x `n` back-to-back calls between device events after a warm-up, median over the rounds:
  forward    under no_grad
  train      forward, a linear loss, backward to x and to the direction map
The plain route is the same module with EQA_VN_ACT_KERNEL=0 (the reference's sequence of torch ops on the device).  The fused
forward moves 2 x numel x 4 bytes (one read of x, one write of y); its bytes/s are that over the median time.
One JSON line per (shape, leg).  --softplus: VNSoftplus instead of VNLeakyReLU(0.2).  --small: tiny shapes and few calls, to rehearse."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import equiadapt_amd as ea

dev = torch.device("cuda:0")
small = "--small" in sys.argv
softplus = "--softplus" in sys.argv
SHAPES = ((2, 21, 3, 64, 20), (2, 85, 3, 64, 1)) if small else ((32, 21, 3, 1024, 20), (32, 85, 3, 1024, 1))
N, ROUNDS = (3, 2) if small else (20, 5)
ENV = "EQA_VN_ACT_KERNEL"


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, n, rounds):
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, n))
    return {k: sorted(v)[len(v) // 2] for k, v in got.items()}, {k: (min(v), max(v)) for k, v in got.items()}


for shape in SHAPES:
    torch.manual_seed(0)
    C = shape[1]
    mod = (ea.VNSoftplus(C) if softplus else ea.VNLeakyReLU(C, negative_slope=0.2)).to(dev)
    x = torch.randn(*shape, device=dev)
    xg = x.clone().requires_grad_(True)
    w = torch.randn(*shape, device=dev)
    routes = {}

    def forward(kernel):
        os.environ[ENV] = "1" if kernel else "0"
        with torch.no_grad():
            y = mod(x)
        routes["forward fused" if kernel else "forward plain"] = mod.last_route
        return y

    def train(kernel):
        os.environ[ENV] = "1" if kernel else "0"
        xg.grad = None
        mod.map_to_dir.weight.grad = None
        y = mod(xg)
        routes["train fused" if kernel else "train plain"] = mod.last_route
        (y * w).sum().backward()
        return xg.grad, mod.map_to_dir.weight.grad

    a, b = forward(True), forward(False)
    diff = float((a - b).abs().max())
    del a, b
    moved = 2 * x.numel() * 4
    med, spread = alternate({"fused": lambda: forward(True), "plain": lambda: forward(False)}, N, ROUNDS)
    print(json.dumps({"shape": shape, "module": type(mod).__name__, "leg": "forward", "fused_ms": med["fused"], "plain_ms": med["plain"],
                      "speedup": med["plain"] / med["fused"], "fused_bytes": moved, "fused_TB_per_s": moved / (med["fused"] * 1e-3) / 1e12,
                      "max_abs_diff_of_outputs": diff, "min_max_ms": spread, "routes": dict(routes)}), flush=True)

    (gxa, gwa), (gxb, gwb) = [tuple(t.clone() for t in train(k)) for k in (True, False)]
    # the two routes round <x, d> differently: where it is within rounding of 0 the LeakyReLU gate falls on different sides and the
    # gradient of that (b, c, p) differs by the size of the gate's jump
    gdiff = (float((gxa - gxb).abs().max()), float((gwa - gwb).abs().max() / gwb.abs().max()), int(((gxa - gxb).abs() > 1e-3).sum()))
    del gxa, gxb
    med, spread = alternate({"fused": lambda: train(True), "plain": lambda: train(False)}, N, ROUNDS)
    print(json.dumps({"shape": shape, "module": type(mod).__name__, "leg": "train", "fused_ms": med["fused"], "plain_ms": med["plain"],
                      "speedup": med["plain"] / med["fused"], "max_abs_diff_gx": gdiff[0], "max_rel_diff_gW": gdiff[1],
                      "gx_entries_differing_by_more_than_1e-3": gdiff[2], "gx_entries": xg.numel(),
                      "min_max_ms": spread, "routes": dict(routes)}), flush=True)
os.environ.pop(ENV, None)
