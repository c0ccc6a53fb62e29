"""The training kernels of ResNet18Network's basic blocks on the device, kernel against library call, same process, alternating:
python tools/kbench_conv3x3_train.py

Shapes: the ten layer forms of the network at the classification recipe's 96 x 96 input and 256 views (G x B) per step -- per stage
the stride-1 3 x 3 layer on its map (24 x 24 x 64, 12 x 12 x 128, 6 x 6 x 256, 3 x 3 x 512, channels-last) and, for stages 2 to 4, the
stride-2 3 x 3 layer and the 1 x 1 stride-2 shortcut from the stage before.  Legs, each `rounds` x `n` back-to-back calls between
device events after a warm-up, median over the rounds:
  wgrad     eqa_conv3x3_wgrad (two launches) against torch.ops.aten.convolution_backward with only the weight mask
  dgrad     eqa_conv3x3_dgrad (packing the filters included: a training step packs them once per step) against the same with only the
            input mask
  bn block  relu(bn(z)), relu(bn(z) + res) and bn(z) with batch statistics, forward + backward: BnResActFunction against
            F.batch_norm + add + relu under autograd, on each stage's map
  network   one training step (forward + backward) of the whole network at the same batch, EQA_RESNET_TRAIN_KERNEL=1 against unset
TFLOP/s from shape-derived counts (2 x output pixels x taps x Cin x Cout).  One JSON line per (shape, leg).  --small: tiny shapes and
few calls, to rehearse."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd import ops
from equiadapt_amd.images.canonicalization_networks.custom_nonequivariant_networks import BnResActFunction

dev = torch.device("cuda:0")
small = "--small" in sys.argv
VIEWS, SIDE = (4, 32) if small else (256, 96)
STAGES = [(VIEWS, SIDE // 4 >> i, 64 << i) for i in range(4)]          # (views, map side, channels)
N, ROUNDS = (3, 2) if small else (20, 5)
ENV = "EQA_RESNET_TRAIN_KERNEL"


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


def report(shape, cout, leg, a, b, med, spread, flop=None, **more):
    row = {"shape": shape, "cout": cout, "leg": leg, a + "_ms": med[a], b + "_ms": med[b], "speedup_over_" + b: med[b] / med[a], "min_max_ms": spread}
    if flop:
        row.update(flop=flop, **{a + "_TFLOP_per_s": flop / (med[a] * 1e-3) / 1e12, b + "_TFLOP_per_s": flop / (med[b] * 1e-3) / 1e12})
    row.update(more)
    print(json.dumps(row), flush=True)


def conv_legs(name, B, side, cin, cout, taps, stride):
    """Both gradients of one layer form: x (B, side, side, cin), dz (B, side / stride, side / stride, cout)."""
    torch.manual_seed(0)
    k, pad = (3, 1) if taps == 9 else (1, 0)
    out = (side + 2 * pad - k) // stride + 1
    x = torch.randn(B, side, side, cin, device=dev)
    w = torch.randn(cout, cin, k, k, device=dev) / (taps * cin) ** 0.5
    dz = torch.randn(B, out, out, cout, device=dev)
    assert ops.conv3x3_wgrad_supported(B, side, side, cin, cout, taps, stride) and ops.conv3x3_dgrad_supported(B, side, side, cin, cout, taps, stride)
    x_cl, dz_cl, w_cl = x.permute(0, 3, 1, 2), dz.permute(0, 3, 1, 2), w.contiguous(memory_format=torch.channels_last)
    flop = 2 * B * out * out * taps * cin * cout

    def lib(mask):
        return torch.ops.aten.convolution_backward(dz_cl, x_cl, w_cl, None, (stride, stride), (pad, pad), (1, 1), False, (0, 0), 1, mask)

    legs = {"wgrad": (lambda: ops.conv3x3_wgrad(x, dz, taps, stride), lambda: lib((False, True, False))[1]),
            "dgrad": (lambda: ops.conv3x3_dgrad(dz, ops.pack_conv3x3_dgrad_weights(w), (side, side), None, taps, stride).permute(0, 3, 1, 2),
                      lambda: lib((True, False, False))[0])}
    for leg, (kernel, library) in legs.items():
        got, want = kernel(), library()
        diff = float((got - want).abs().max())
        med, spread = alternate({"kernel": kernel, "library": library}, N, ROUNDS)
        report((B, side, side, cin), cout, f"{name}:{leg}", "kernel", "library", med, spread, flop, max_abs_diff_of_outputs=diff,
               max_abs_output=float(want.abs().max()))


def bn_legs(B, side, C, forms):
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    z = torch.randn(B, side, side, C, device=dev, requires_grad=True)
    res = torch.randn(B, side, side, C, device=dev, requires_grad=True)
    gy = torch.randn(B, side, side, C, device=dev)
    for name, has_res, relu in forms:
        def kernel():
            z.grad = res.grad = None
            BnResActFunction.apply(z, bn.weight, bn.bias, bn, res if has_res else None, relu).backward(gy)
            return z.grad

        def library():
            z.grad = res.grad = None
            t = F.batch_norm(z.permute(0, 3, 1, 2), bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, bn.eps)
            if has_res:
                t = t + res.permute(0, 3, 1, 2)
            (F.relu(t) if relu else t).backward(gy.permute(0, 3, 1, 2))
            return z.grad

        diff = float((kernel() - library()).abs().max())
        med, spread = alternate({"kernel": kernel, "library": library}, N, ROUNDS)
        report((B, side, side, C), C, f"bn:{name}", "kernel", "library", med, spread, max_abs_diff_of_dz=diff)


for i, (B, side, C) in enumerate(STAGES):
    conv_legs("conv3x3", B, side, C, C, 9, 1)
    if i:
        conv_legs("conv3x3s2", B, 2 * side, C // 2, C, 9, 2)
        conv_legs("conv1x1s2", B, 2 * side, C // 2, C, 1, 2)
for i, (B, side, C) in enumerate(STAGES):
    bn_legs(B, side, C, [("relu(bn)", False, True), ("relu(bn+res)", True, True)] + ([("bn", False, False)] if i else []))

torch.manual_seed(0)
net = ea.ResNet18Network((3, SIDE, SIDE), 8, 3).to(dev).train()
x = torch.randn(VIEWS, 3, SIDE, SIDE, device=dev)
wgt = torch.randn(VIEWS, 128, device=dev)
routes = {}


def step(on):
    if on:
        os.environ[ENV] = "1"
    else:
        os.environ.pop(ENV, None)
    net.zero_grad(set_to_none=True)
    y = net(x)
    (y * wgt).sum().backward()
    routes["kernels" if on else "plain"] = (list(net.last_routes), list(net.last_wgrad_routes))
    return y.detach()


diff = float((step(True) - step(False)).abs().max())
med, spread = alternate({"kernels": lambda: step(True), "plain": lambda: step(False)}, max(N // 4, 2), ROUNDS)
report(tuple(x.shape), 128, "network:training step", "kernels", "plain", med, spread, max_abs_diff_of_outputs=diff, routes=routes)
os.environ.pop(ENV, None)
