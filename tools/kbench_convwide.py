"""The convolutions of WideResNet50Network on the device, kernel against torch ops, same process, alternating:
python tools/kbench_convwide.py [forms | network] [--small]

Shapes: the network at the classification recipe's 96 x 96 input and 256 views (G x B) per step: maps of 24 x 24, 12 x 12, 6 x 6 and
3 x 3 behind the stem, channels-last.  Each leg is `rounds` x `n` back-to-back calls between device events after a warm-up, median
over the rounds (the method of tools/kbench_conv3x3.py).
  forms    each of the 23 distinct (Cin, Cout, k, stride) forms behind the stem at the first map it meets, as the network calls it
           (conv1 and conv2 with ReLU, conv3 with residual and ReLU, the projection bare): eqa_convwide_nhwc at the library-chosen
           ksplit, at ksplit 1 and at half and twice the chosen value where admitted, against the torch-op sequence it replaces
           (F.conv2d with the folded filters and bias on the same channels-last memory, add_, relu_)
  network  WideResNet50Network in eval under no_grad at the same batch: plain (EQA_WIDERESNET_KERNEL=0), fused without a gate (every
           admitted layer on the kernel) and fused with the gate `_kernel_pays`
Without an argument the parent process runs each part as a child of its own under `timeout`, one after the other, and stops at the
first that fails.  TFLOP/s from shape-derived counts (2 x output pixels x taps x Cin x Cout).  One JSON line per leg.  --small: tiny
shapes and few calls, to rehearse."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = {"forms": 420, "network": 240}                     # seconds each child may take

args = [a for a in sys.argv[1:] if not a.startswith("--")]
small = "--small" in sys.argv
if not args:
    for part, limit in PARTS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), part] + (["--small"] if small else [])
        status = subprocess.run(cmd).returncode
        if status != 0:
            sys.exit(f"kbench_convwide: part {part!r} ended with status {status}; nothing further is started")
    sys.exit(0)

import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd import ops

dev = torch.device("cuda:0")
VIEWS, SIDE = (4, 32) if small else (256, 96)
N, ROUNDS = (3, 2) if small else (20, 5)
ENV = "EQA_WIDERESNET_KERNEL"


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


def forms():
    """(route, side of the input map, cin, cout, taps, stride) of every distinct form, in the order the network meets them."""
    out, seen, cin, side = [], set(), 64, SIDE // 4
    for li, planes in enumerate((64, 128, 256, 512)):
        width, cout = 2 * planes, 4 * planes
        for bi in range(2):                                 # the first block and one behind it: every form of the layer
            stride = 2 if (bi == 0 and li > 0) else 1
            layers = [("conv1x1", side, cin, width, 1, 1), ("conv3x3", side, width, width, 9, stride)]
            if bi == 0:
                layers.append(("proj", side, cin, cout, 1, stride))
            side = (side - 1) // stride + 1
            layers.append(("conv1x1+res", side, width, cout, 1, 1))
            for f in layers:
                if f[2:] not in seen:
                    seen.add(f[2:])
                    out.append(f)
            cin = cout
    return out


def leg(route, B, side, cin, cout, taps, stride):
    torch.manual_seed(0)
    k, pad = (3, 1) if taps == 9 else (1, 0)
    x = torch.randn(B, side, side, cin, device=dev)
    w = torch.randn(cout, cin, k, k, device=dev) / (taps * cin) ** 0.5
    bias = torch.randn(cout, device=dev)
    o = (side + 2 * pad - k) // stride + 1
    with_res, relu = route == "conv1x1+res", route != "proj"
    res = torch.randn(B, o, o, cout, device=dev) if with_res else None
    shape = (B, side, side, cin, cout, taps, stride)
    assert ops.convwide_supported(*shape)
    wpk = ops.pack_conv3x3_weights(w)
    x_cl, w_cl = x.permute(0, 3, 1, 2), w.contiguous(memory_format=torch.channels_last)       # the same memory as channels-last NCHW
    res_cl = res.permute(0, 3, 1, 2) if with_res else None
    chosen, top = ops.convwide_ksplit(*shape), min(16, taps * cin // 32)
    splits = sorted({ks for ks in (1, chosen // 2, chosen, 2 * chosen) if 1 <= ks <= top})

    def kernel(ks):
        return lambda: ops.convwide_nhwc(x, wpk, bias, res, relu, taps, stride, ks)

    def torch_ops():
        z = F.conv2d(x_cl, w_cl, bias, stride, pad)
        if with_res:
            z.add_(res_cl)
        return z.relu_() if relu else z

    diff = float((kernel(chosen)() - torch_ops().permute(0, 2, 3, 1)).abs().max())
    flop = 2 * B * o * o * taps * cin * cout
    fns = {f"ksplit{ks}": kernel(ks) for ks in splits}
    fns["torch_ops"] = torch_ops
    med, spread = alternate(fns, N, ROUNDS)
    best = min(splits, key=lambda ks: med[f"ksplit{ks}"])
    print(json.dumps({"leg": route, "shape": (B, side, side, cin), "cout": cout, "taps": taps, "stride": stride, "pixels": B * o * o,
                      "ksplit_chosen": chosen, "ms": med, "kernel_ms": med[f"ksplit{chosen}"], "torch_ops_ms": med["torch_ops"],
                      "speedup_over_torch_ops": med["torch_ops"] / med[f"ksplit{chosen}"], "ksplit_best": best,
                      "kernel_TFLOP_per_s": flop / (med[f"ksplit{chosen}"] * 1e-3) / 1e12,
                      "torch_ops_TFLOP_per_s": flop / (med["torch_ops"] * 1e-3) / 1e12, "flop": flop, "max_abs_diff_of_outputs": diff,
                      "min_max_ms": spread}), flush=True)


def network():
    torch.manual_seed(0)
    net = ea.WideResNet50Network((3, SIDE, SIDE), 8, 3).to(dev).eval()
    x = torch.randn(VIEWS, 3, SIDE, SIDE, device=dev)
    gate = type(net)._kernel_pays
    routes = {}

    def run(way):
        os.environ[ENV] = "0" if way == "plain" else "1"
        type(net)._kernel_pays = staticmethod((lambda *a: True) if way == "fused_no_gate" else gate)
        y = net(x)
        routes[way] = list(net.last_routes)
        return y

    ways = ("plain", "fused_no_gate", "fused")
    outs = {w: run(w) for w in ways}
    med, spread = alternate({w: (lambda w=w: run(w)) for w in ways}, max(N // 4, 2), ROUNDS)
    type(net)._kernel_pays = staticmethod(gate)
    os.environ.pop(ENV, None)
    print(json.dumps({"leg": "network", "input": tuple(x.shape), "ms": med, "speedup_no_gate": med["plain"] / med["fused_no_gate"],
                      "speedup_gated": med["plain"] / med["fused"], "max_abs_output": float(outs["plain"].abs().max()),
                      "max_abs_diff_no_gate": float((outs["fused_no_gate"] - outs["plain"]).abs().max()),
                      "max_abs_diff_gated": float((outs["fused"] - outs["plain"]).abs().max()), "min_max_ms": spread,
                      "lib_layers_gated": routes["fused"].count("lib") - 1, "ksplits": list(net.last_ksplits), "routes": routes}), flush=True)


with torch.no_grad():
    if args[0] == "forms":
        for f in forms():
            leg(f[0], VIEWS, *f[1:])
    elif args[0] == "network":
        network()
    else:
        sys.exit(f"kbench_convwide: unknown part {args[0]!r}")
