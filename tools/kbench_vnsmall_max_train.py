"""One training step (forward + backward) of VNSmall(pooling="max") at B = 64, N = 1024, k = 20, HIP events:
python tools/kbench_vnsmall_max_train.py [--out FILE]
  * the whole step on the fused first block (EQA_TRAIN_FAST unset) and on the op-by-op block (EQA_TRAIN_FAST=0), alternating,
    several windows each (the spread is printed);
  * eqa_vn_convpos_max_fwd, _max_bwd_reduce, _max_bwd_apply alone, beside the mean pooling's three at the same shape.
Prints a markdown table (and writes it to --out)."""
import argparse
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import equiadapt_amd as ea  # noqa: E402
from equiadapt_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()

lib = _lib.load()
assert torch.cuda.is_available(), "a timing needs the GPU"
dev = torch.device("cuda:0")
B, N, k = args.batch, 1024, 20


def ev_time(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


torch.manual_seed(0)
net = ea.VNSmall(types.SimpleNamespace(n_knn=k, pooling="max")).to(dev).train()
x = torch.randn(B, 3, N, device=dev)


def step():
    for p in net.parameters():
        p.grad = None
    net(x).sum().backward()


lines = [f"`VNSmall(pooling=\"max\")`, one training step (forward + backward), B = {B}, N = {N}, k = {k}; HIP events, ms per step,",
         "five alternating windows per route:", "", "| first block | windows (ms) | median (ms) |", "|---|---|---|"]
windows = {"fused": [], "op by op": []}
for w in range(5):
    for name, env, reps in (("fused", None, 50), ("op by op", "0", 10)):
        if env is None:
            os.environ.pop("EQA_TRAIN_FAST", None)
        else:
            os.environ["EQA_TRAIN_FAST"] = env
        windows[name].append(ev_time(step, reps, 3))
os.environ.pop("EQA_TRAIN_FAST", None)
for name, v in windows.items():
    lines.append(f"| {name} | {', '.join(f'{t:.3f}' for t in v)} | {sorted(v)[len(v) // 2]:.3f} |")
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
step()
torch.cuda.synchronize()
lines += ["", f"Peak allocation of the fused step beyond the network and the cloud: {(torch.cuda.max_memory_allocated() - base) / 1e6:.1f} MB "
          f"(one (B, 21, 3, N, k) fp32 tensor: {B * 63 * N * k * 4 / 1e6:.0f} MB)."]

# the kernels alone
cp = net.conv_pos
Wf, Wd, Wp = (w.detach().contiguous() for w in (cp.map_to_feat.weight, cp.map_to_dir.weight, net.pool.map_to_dir.weight))
idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
_lib.check(lib.eqa_vn_knn(x.data_ptr(), idx.data_ptr(), B, N, k, None), "eqa_vn_knn")
stat = torch.zeros(128, device=dev)
stat[0:21], stat[96:117] = 1.0, 1.0                         # scale = rstd = 1, shift = mean = 0
scale, shift, mean, rstd = stat[0:21], stat[32:53], stat[64:85], stat[96:117]
red = torch.full((64,), 1e-3, device=dev)
pooled = torch.empty(B, 21, 3, N, device=dev)
sel = torch.empty(B, 21, N, dtype=torch.uint8, device=dev)
g = torch.randn(B, 21, 3, N, device=dev)
nblk = B * lib.eqa_vn_blocks(N)
part = torch.empty(nblk, 21, 6, device=dev)
P = lambda t: t.data_ptr()  # noqa: E731
common = (P(x), P(idx), P(Wf), P(Wd), P(scale), P(shift))
kernels = {
    "eqa_vn_convpos_max_fwd": lambda: lib.eqa_vn_convpos_max_fwd(*common, P(Wp), P(pooled), P(sel), B, N, k, None),
    "eqa_vn_convpos_max_bwd_reduce": lambda: lib.eqa_vn_convpos_max_bwd_reduce(*common, P(mean), P(rstd), P(g), P(sel), P(part), B, N, k, None),
    "eqa_vn_convpos_max_bwd_apply": lambda: lib.eqa_vn_convpos_max_bwd_apply(*common, P(mean), P(rstd), P(red), P(red[32:]), P(g), P(sel),
                                                                            P(part), B, N, k, None),
    "eqa_vn_convpos_fwd (mean)": lambda: lib.eqa_vn_convpos_fwd(*common, P(pooled), B, N, k, None),
    "eqa_vn_convpos_bwd_reduce (mean)": lambda: lib.eqa_vn_convpos_bwd_reduce(*common, P(mean), P(rstd), P(g), P(part), B, N, k, None),
    "eqa_vn_convpos_bwd_apply (mean)": lambda: lib.eqa_vn_convpos_bwd_apply(*common, P(mean), P(rstd), P(red), P(red[32:]), P(g), P(part),
                                                                           B, N, k, None),
}
lines += ["", "The kernels alone (200 launches per window, three windows, us per launch):", "", "| kernel | windows (us) |", "|---|---|"]
assert kernels["eqa_vn_convpos_max_fwd"]() == 0              # sel is written before the backward kernels read it
for name, fn in kernels.items():
    assert fn() == 0, name
    lines.append(f"| `{name}` | {', '.join(f'{ev_time(fn, 200, 5) * 1e3:.1f}' for _ in range(3))} |")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
