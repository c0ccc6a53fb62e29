"""The steerable lifting kernels alone, and the steerable.yaml network's eval forward and training step with and without them:
python tools/kbench_steer_lift.py [--small] [--net-only]

1. Per shape class -- the configuration's first layer (B = 256, 3 x 96 x 96 -> 144 x 90 x 90, k = 7, 16 fields) and the grayscale
   one (B = 256, 1 x 28 x 28 -> 144 x 24 x 24, k = 5, 16 fields) -- alternating, back to back:
     clone            torch's clone() of the output map: the byte yardstick (one map read, one written)
     steer_lift       eqa_steer_lift_fwd without / with the epilogue statistics (folded to the (fields, 6) sums)
     lib              the parent's route of the same layer: F.conv2d on the channels-last bank (what EQA_STEER_LIFT_KERNEL=0 runs);
                      lib_stats: followed by ops.field_norm_stats of its output, the parent's training forward
     wgrad            eqa_steer_lift_wgrad against torch.nn.grad.conv2d_weight
   TFLOPs: 2 B OH OW 9F Cin k^2 / time, against the 157.3 TFLOP/s fp32 matrix peak.
2. ESCNNSteerableNetwork((3, 96, 96), 16 fields, k = 7, 3 layers) at B = 256: eval forward under no_grad and training step
   (forward + backward of (out * w).sum()), EQA_STEER_LIFT_KERNEL unset against "0", alternating, with the library's launches.
One JSON line per measurement: medians of 5 x 20 (kernels) / 5 x 3 (network) with the (min, max) of the rounds.  --small: toy sizes,
to rehearse the script."""
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
KNOB = "EQA_STEER_LIFT_KERNEL"
PEAK_TFLOPS = 157.3


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


def layer(B, cin, hw, k, fields):
    x = torch.randn(B, cin, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
    bank = (torch.randn(9 * fields, cin, k, k, device=dev) / (cin * k * k) ** 0.5).contiguous(memory_format=torch.channels_last)
    wpk = ops.pack_steer_lift_weights(bank)
    y, _ = ops.steer_lift(x, wpk, k, fields)
    dy = torch.randn_like(y)
    ref = F.conv2d(x, bank)
    err = float((y - ref).abs().max() / ref.abs().max())
    gref = torch.nn.grad.conv2d_weight(x, bank.shape, dy)
    gerr = float((ops.steer_lift_wgrad(x, dy, k) - gref).abs().max() / gref.abs().max())
    del ref, gref
    med, spread = alternate({"clone": lambda: y.clone(),
                             "steer_lift": lambda: ops.steer_lift(x, wpk, k, fields),
                             "steer_lift_stats": lambda: ops.steer_lift(x, wpk, k, fields, with_stats=True),
                             "lib": lambda: F.conv2d(x, bank),
                             "lib_stats": lambda: ops.field_norm_stats(F.conv2d(x, bank).contiguous(memory_format=torch.channels_last)).sum(0),
                             "wgrad": lambda: ops.steer_lift_wgrad(x, dy, k),
                             "lib_wgrad": lambda: torch.nn.grad.conv2d_weight(x, bank.shape, dy)}, n=20, rounds=5)
    flop = 2.0 * y.numel() * cin * k * k
    tf = {name: flop / med[name] / 1e9 for name in ("steer_lift", "steer_lift_stats", "lib", "wgrad", "lib_wgrad")}
    print(json.dumps({"what": "steer_lift kernels", "x": list(x.shape), "y": list(y.shape), "k": k, "map_GB": round(y.numel() * 4 / 1e9, 3),
                      "median_ms": med, "min_max_ms": spread, "TFLOPs": tf,
                      "frac_of_fp32_matrix_peak": {name: v / PEAK_TFLOPS for name, v in tf.items()},
                      "fwd_speedup_over_lib": med["lib"] / med["steer_lift"], "fwd_stats_speedup_over_lib": med["lib_stats"] / med["steer_lift_stats"],
                      "wgrad_speedup_over_lib": med["lib_wgrad"] / med["wgrad"], "rel_diff_fwd": err, "rel_diff_wgrad": gerr}), flush=True)


if "--net-only" not in sys.argv:
    layer(4 if small else 256, 3, 40 if small else 96, 7, 16)
    torch.cuda.empty_cache()
    layer(4 if small else 256, 1, 28, 5, 16)
    torch.cuda.empty_cache()

B, hw = (4, 48) if small else (256, 96)
torch.manual_seed(0)
net = ea.ESCNNSteerableNetwork((3, hw, hw), 16, 7, "rotation", 3).to(dev)
img = torch.randn(B, 3, hw, hw, device=dev)
w = torch.randn(B, 2, 2, device=dev)


def knob_env(on):
    if on:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = "0"


def forward(on):
    knob_env(on)
    with torch.no_grad():
        return net(img)


def step(on):
    knob_env(on)
    net.zero_grad(set_to_none=True)
    out = net(img)
    (out * w).sum().backward()
    return out.detach()


def launches(fn):
    got = {}
    for on in (True, False):
        with ops.KernelTimer() as t:
            fn(on)
        got["on" if on else "off"] = {"routes": list(net.last_routes), **{k: [v[0], round(v[1], 4)] for k, v in t.summary().items()}}
    return got


net.eval()
ref, got = forward(False), forward(True)
err = float((got - ref).abs().max() / ref.abs().max())
med, spread = alternate({"on": lambda: forward(True), "off": lambda: forward(False)}, n=3, rounds=5)
print(json.dumps({"what": "steerable.yaml network eval forward", "B": B, "hw": hw, "on_ms": med["on"], "off_ms": med["off"],
                  "speedup": med["off"] / med["on"], "rel_diff_of_outputs": err, "min_max_ms": spread,
                  "library_launches_count_mean_ms": launches(forward)}), flush=True)

net.train()
ref, got = step(False), step(True)
err = float((got - ref).abs().max() / ref.abs().max())
grads = {k: p.grad.clone() for k, p in net.named_parameters()}
step(False)
gerr = max(float((p.grad - grads[k]).abs().max() / grads[k].abs().max().clamp_min(1e-30)) for k, p in net.named_parameters())
med, spread = alternate({"on": lambda: step(True), "off": lambda: step(False)}, n=3, rounds=5)
print(json.dumps({"what": "steerable.yaml network training step", "B": B, "hw": hw, "on_ms": med["on"], "off_ms": med["off"],
                  "speedup": med["off"] / med["on"], "rel_diff_of_outputs": err, "rel_diff_of_gradients": gerr, "min_max_ms": spread,
                  "library_launches_count_mean_ms": launches(step)}), flush=True)
knob_env(True)
