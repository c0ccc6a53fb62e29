"""The bottleneck junction of ESCNNWRNEquivariantNetwork on the device, kernel against torch ops, same process, alternating:
python tools/kbench_gconv1x1.py

Shapes: the three bottleneck stages of the reference's segmentation recipe (k = 5, out_channels = 64, 12 layers, C4, 128 x 128 input)
at B = 8: 124 x 124 x 64, 116 x 116 x 128, 108 x 108 x 256 channels-last.  Legs, each `rounds` x `n` back-to-back calls between
device events after a warm-up, median over the rounds:
  junction   y = relu(s (conv1x1(u) + bias + h) + t): eqa_gconv1x1_nhwc (one launch) against the torch-op sequence the network runs
             where the kernel does not take a shape (F.conv2d with bias, add_, mul_, add_, relu_), and against a clone() that moves
             the same bytes (the junction reads u and h and writes y: three maps; the clone reads and writes 1.5 maps)
  network    the whole recipe network in eval under no_grad, fused route against plain route (EQA_WRN_KERNEL=0)
  wgrad      the filter and bias gradient of the 1 x 1 convolution at the same maps: eqa_gconv1x1_wgrad against dz.t() @ x on the
             library GEMM
  train_step one forward + backward of the recipe network in train(): training route against plain route (EQA_WRN_KERNEL=0)
One JSON line per (shape, leg).  --small: tiny shapes and few calls, to rehearse."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd import ops

dev = torch.device("cuda:0")
small = "--small" in sys.argv
SHAPES = ((2, 64, 12, 12), (2, 128, 10, 10)) if small else ((8, 64, 124, 124), (8, 128, 116, 116), (8, 256, 108, 108))
N, ROUNDS = (3, 2) if small else (20, 5)
ENV = "EQA_WRN_KERNEL"


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


with torch.no_grad():
    for shape in SHAPES:
        torch.manual_seed(0)
        B, C, H, W = shape
        u = torch.randn(*shape, device=dev).contiguous(memory_format=torch.channels_last)
        h = torch.randn(*shape, device=dev).contiguous(memory_format=torch.channels_last)
        bank = (torch.randn(C, C, 1, 1, device=dev) / C ** 0.5).contiguous(memory_format=torch.channels_last)
        bias, s, t = torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        wpk = ops.pack_gconv1x1_weights(bank)
        flat = torch.randn(3 * u.numel() // 2, device=dev)
        assert ops.gconv1x1_supported(B * H * W, C, C)

        def kernel():
            return ops.gconv1x1_nhwc(u, wpk, bias, h, s, t, True)

        def torch_ops():
            z = F.conv2d(u, bank, bias).add_(h)
            return torch.relu_(z.mul_(s[None, :, None, None]).add_(t[None, :, None, None]))

        diff = float((kernel() - torch_ops()).abs().max())
        moved = 3 * u.numel() * 4
        med, spread = alternate({"kernel": kernel, "torch_ops": torch_ops, "clone": flat.clone}, N, ROUNDS)
        print(json.dumps({"shape": shape, "leg": "junction", "kernel_ms": med["kernel"], "torch_ops_ms": med["torch_ops"],
                          "clone_ms": med["clone"], "speedup_over_torch_ops": med["torch_ops"] / med["kernel"],
                          "clone_over_kernel": med["clone"] / med["kernel"], "bytes": moved,
                          "kernel_TB_per_s": moved / (med["kernel"] * 1e-3) / 1e12, "kernel_TFLOP_per_s": 2 * u.numel() * C / (med["kernel"] * 1e-3) / 1e12,
                          "max_abs_diff_of_outputs": diff, "min_max_ms": spread}), flush=True)
        del u, h, flat

    torch.manual_seed(0)
    cfg = ((3, 40, 40), 32, 5, "rotation", 6, 4) if small else ((3, 128, 128), 64, 5, "rotation", 12, 4)
    net = ea.ESCNNWRNEquivariantNetwork(*cfg).to(dev).eval()
    x = torch.randn(2 if small else 8, *cfg[0], device=dev)
    routes = {}

    def run(fused):
        os.environ[ENV] = "1" if fused else "0"
        y = net(x)
        routes["fused" if fused else "plain"] = list(net.last_routes)
        return y

    a, b = run(True), run(False)
    diff = float((a - b).abs().max())
    med, spread = alternate({"fused": lambda: run(True), "plain": lambda: run(False)}, max(N // 4, 2), ROUNDS)
    print(json.dumps({"config": cfg, "batch": x.shape[0], "leg": "network", "fused_ms": med["fused"], "plain_ms": med["plain"],
                      "speedup": med["plain"] / med["fused"], "max_abs_diff_of_outputs": diff, "max_abs_output": float(b.abs().max()),
                      "min_max_ms": spread, "routes": routes}), flush=True)
os.environ.pop(ENV, None)


def train_legs():
    """wgrad: eqa_gconv1x1_wgrad (filter and bias gradient, two launches) against dz.t() @ x on the library GEMM (which leaves the
    bias gradient out) at the same three maps.  train_step: forward + backward of the recipe network in train(), the training route
    against the plain route (EQA_WRN_KERNEL=0)."""
    for shape in SHAPES:
        torch.manual_seed(0)
        B, C, H, W = shape
        P = B * H * W
        x, dz = torch.randn(P, C, device=dev), torch.randn(P, C, device=dev)
        assert ops.gconv1x1_wgrad_supported(P, C, C)
        ref = dz.double().t() @ x.double()
        err_k = float((ops.gconv1x1_wgrad(x, dz)[0].view(C, C).double() - ref).abs().max())
        err_l = float(((dz.t() @ x).double() - ref).abs().max())
        med, spread = alternate({"kernel": lambda: ops.gconv1x1_wgrad(x, dz), "library_gemm": lambda: dz.t() @ x}, N, ROUNDS)
        print(json.dumps({"shape": shape, "leg": "wgrad", "kernel_ms": med["kernel"], "library_gemm_ms": med["library_gemm"],
                          "speedup_over_library_gemm": med["library_gemm"] / med["kernel"],
                          "kernel_TFLOP_per_s": 2 * P * C * C / (med["kernel"] * 1e-3) / 1e12,
                          "kernel_TB_per_s": 2 * P * C * 4 / (med["kernel"] * 1e-3) / 1e12,
                          "max_abs_err_to_fp64": {"kernel": err_k, "library_gemm": err_l}, "min_max_ms": spread}), flush=True)
        del x, dz, ref

    torch.manual_seed(0)
    cfg = ((3, 40, 40), 32, 5, "rotation", 6, 4) if small else ((3, 128, 128), 64, 5, "rotation", 12, 4)
    net = ea.ESCNNWRNEquivariantNetwork(*cfg).to(dev).train()
    x = torch.randn(2 if small else 8, *cfg[0], device=dev)
    routes = {}

    def step(fused):
        os.environ[ENV] = "1" if fused else "0"
        net.zero_grad(set_to_none=True)
        y = net(x)
        routes["train" if fused else "plain"] = list(net.last_routes)
        y.square().sum().backward()
        return y.detach()

    a, b = step(True), step(False)
    med, spread = alternate({"train": lambda: step(True), "plain": lambda: step(False)}, max(N // 4, 2), ROUNDS)
    print(json.dumps({"config": cfg, "batch": x.shape[0], "leg": "train_step", "train_route_ms": med["train"], "plain_ms": med["plain"],
                      "speedup": med["plain"] / med["train"], "max_abs_diff_of_outputs": float((a - b).abs().max()),
                      "max_abs_output": float(b.abs().max()), "min_max_ms": spread, "routes": routes}), flush=True)
    os.environ.pop(ENV, None)


train_legs()
