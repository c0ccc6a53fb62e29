"""The 3 x 3 convolutions of ResNet18Network on the device, kernel against torch ops, same process, alternating:
python tools/kbench_conv3x3.py

Shapes: the four stages of the network at the classification recipe's 96 x 96 input and 256 views (G x B) per step: maps of
24 x 24 x 64, 12 x 12 x 128, 6 x 6 x 256 and 3 x 3 x 512, channels-last.  Legs, each `rounds` x `n` back-to-back calls between device
events after a warm-up, median over the rounds:
  conv3x3+res  a block's second layer, y = relu(conv3x3(x) + bias + res), stride 1: eqa_conv3x3_nhwc (one launch) against the
               torch-op sequence it replaces (F.conv2d with the folded filters and bias on a channels-last map, add_, relu_)
  conv3x3s2    a stage's first layer, y = relu(conv3x3(x) + bias) at stride 2 from the stage before (stages 2 to 4): against
               F.conv2d + relu_
  conv1x1s2    the projection shortcut of that block, y = conv1x1(x) + bias at stride 2: against F.conv2d
  network      the whole network in eval under no_grad at the same batch, fused route against plain route (EQA_RESNET_KERNEL=0)
TFLOP/s from shape-derived counts (2 x output pixels x taps x Cin x Cout).  One JSON line per (shape, leg).  --small: tiny shapes
and few calls, to rehearse."""
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
VIEWS, SIDE = (4, 32) if small else (256, 96)
STAGES = [(VIEWS, SIDE // 4 >> i, 64 << i) for i in range(4)]          # (views, map side, channels)
N, ROUNDS = (3, 2) if small else (20, 5)
ENV = "EQA_RESNET_KERNEL"


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


def leg(name, B, side, cin, cout, taps, stride, with_res):
    """One layer form at one map: x (B, side, side, cin) -> (B, side / stride, side / stride, cout)."""
    torch.manual_seed(0)
    k, pad = (3, 1) if taps == 9 else (1, 0)
    x = torch.randn(B, side, side, cin, device=dev)
    w = torch.randn(cout, cin, k, k, device=dev) / (taps * cin) ** 0.5
    bias = torch.randn(cout, device=dev)
    out = (side + 2 * pad - k) // stride + 1
    res = torch.randn(B, out, out, cout, device=dev) if with_res else None
    relu = taps == 9
    assert ops.conv3x3_supported(B, side, side, cin, cout, taps, stride)
    wpk = ops.pack_conv3x3_weights(w)
    x_cl, w_cl = x.permute(0, 3, 1, 2), w.contiguous(memory_format=torch.channels_last)       # the same memory as channels-last NCHW
    res_cl = res.permute(0, 3, 1, 2) if with_res else None

    def kernel():
        return ops.conv3x3_nhwc(x, wpk, bias, res, relu, taps, stride)

    def torch_ops():
        z = F.conv2d(x_cl, w_cl, bias, stride, pad)
        if with_res:
            z.add_(res_cl)
        return z.relu_() if relu else z

    diff = float((kernel() - torch_ops().permute(0, 2, 3, 1)).abs().max())
    flop = 2 * B * out * out * taps * cin * cout
    med, spread = alternate({"kernel": kernel, "torch_ops": torch_ops}, N, ROUNDS)
    print(json.dumps({"shape": (B, side, side, cin), "cout": cout, "leg": name, "kernel_ms": med["kernel"], "torch_ops_ms": med["torch_ops"],
                      "speedup_over_torch_ops": med["torch_ops"] / med["kernel"], "flop": flop,
                      "kernel_TFLOP_per_s": flop / (med["kernel"] * 1e-3) / 1e12, "torch_ops_TFLOP_per_s": flop / (med["torch_ops"] * 1e-3) / 1e12,
                      "max_abs_diff_of_outputs": diff, "min_max_ms": spread}), flush=True)


with torch.no_grad():
    for i, (B, side, C) in enumerate(STAGES):
        leg("conv3x3+res", B, side, C, C, 9, 1, True)
        if i:
            leg("conv3x3s2", B, 2 * side, C // 2, C, 9, 2, False)
            leg("conv1x1s2", B, 2 * side, C // 2, C, 1, 2, False)

    torch.manual_seed(0)
    net = ea.ResNet18Network((3, SIDE, SIDE), 8, 3).to(dev).eval()
    x = torch.randn(VIEWS, 3, SIDE, SIDE, device=dev)
    routes = {}

    def run(fused):
        os.environ[ENV] = "1" if fused else "0"
        y = net(x)
        routes["fused" if fused else "plain"] = list(net.last_routes)
        return y

    a, b = run(True), run(False)
    diff = float((a - b).abs().max())
    med, spread = alternate({"fused": lambda: run(True), "plain": lambda: run(False)}, max(N // 4, 2), ROUNDS)
    print(json.dumps({"input": tuple(x.shape), "leg": "network", "fused_ms": med["fused"], "plain_ms": med["plain"],
                      "speedup": med["plain"] / med["fused"], "max_abs_diff_of_outputs": diff, "max_abs_output": float(b.abs().max()),
                      "min_max_ms": spread, "routes": routes}), flush=True)
os.environ.pop(ENV, None)
