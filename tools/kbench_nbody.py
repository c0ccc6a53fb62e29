"""VNDeepSets on the device, fused route against plain route, same process, alternating: python tools/kbench_nbody.py

The reference configuration (examples/nbody/configs/canonicalization/vndeepsets.yaml: hidden_dim 16, 4 layers, relu, "p", mean / mean,
dropout 0.5) at S = 100 systems (the reference batch) and S = 4096.  Legs, each `rounds` x `n` back-to-back calls between device
events after a warm-up, median over the rounds:
  inference   eval mode under no_grad
  train       train mode: forward (each route draws its own dropout mask), a linear loss, backward to the parameters
  edges       the fused inference call with the cached pair of complete_graph_edges (hit) against freshly cloned edge tensors every
              call (miss: adjacency kernel + one 4-byte read back)
  canonicalizer step   EuclideanGroupNBody(VNDeepSets) in train mode: forward, invert_canonicalization of a prediction made from the
              canonical coordinates, a linear loss, backward to the parameters; the network on its fused route both times, the frame
              chain behind it on its kernels against EQA_NBODY_FRAME_KERNEL=0 (op by op)
and the number of device launches (kernels, fills, copies) per call of both routes, counted by torch.profiler.
One JSON line per (size, leg).  --small: S = 8 and few calls, to rehearse the script."""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import equiadapt_amd as ea
from equiadapt_amd.nbody import complete_graph_edges

dev = torch.device("cuda:0")
small = "--small" in sys.argv
SIZES = (8,) if small else (100, 4096)
N, ROUNDS = (5, 2) if small else (100, 5)


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
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timed(f, n))
    return {k: sorted(v)[len(v) // 2] for k, v in got.items()}, {k: (min(v), max(v)) for k, v in got.items()}


def launches(fn):
    """Device-side events of one call (after a warm-up call), or a note where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as exc:  # noqa: BLE001
        return f"unavailable: {type(exc).__name__}"


for S in SIZES:
    hp = types.SimpleNamespace(hidden_dim=16, num_layers=4, nonlinearity="relu", canon_feature="p", canon_translation=False,
                               angular_feature=0, layer_pooling="mean", final_pooling="mean", out_dim=4, dropout=0.5, batch_size=S)
    torch.manual_seed(0)
    net = ea.VNDeepSets(hp, device=dev).to(dev)
    M = 5 * S
    loc, vel, charges = torch.randn(M, 3, device=dev), torch.randn(M, 3, device=dev), torch.ones(M, 1, device=dev)
    edges = complete_graph_edges(S, 5, dev)
    wr, wt = torch.randn(M, 3, 3, device=dev), torch.randn(M, 3, device=dev)
    routes = {}

    def infer(kernel, use_edges=None):
        os.environ["EQA_NBODY_KERNEL"] = "1" if kernel else "0"
        net.eval()
        with torch.no_grad():
            out = net(None, loc, use_edges or edges, vel, None, charges)
        routes["inference fused" if kernel else "inference plain"] = net.last_route
        return out

    def train(kernel):
        os.environ["EQA_NBODY_KERNEL"] = "1" if kernel else "0"
        net.train()
        for p in net.parameters():
            p.grad = None
        rot, trans = net(None, loc, edges, vel, None, charges)
        routes["train fused" if kernel else "train plain"] = net.last_route
        ((rot * wr).sum() + (trans * wt).sum()).backward()

    a, b = infer(True), infer(False)
    diff = float((a[0] - b[0]).abs().max())
    med, spread = alternate({"fused": lambda: infer(True), "plain": lambda: infer(False)}, N, ROUNDS)
    print(json.dumps({"S": S, "leg": "inference", "fused_ms": med["fused"], "plain_ms": med["plain"], "speedup": med["plain"] / med["fused"],
                      "launches_fused": launches(lambda: infer(True)), "launches_plain": launches(lambda: infer(False)),
                      "max_abs_diff_of_outputs": diff, "min_max_ms": spread, "routes": dict(routes)}))

    med, spread = alternate({"fused": lambda: train(True), "plain": lambda: train(False)}, N, ROUNDS)
    print(json.dumps({"S": S, "leg": "train", "fused_ms": med["fused"], "plain_ms": med["plain"], "speedup": med["plain"] / med["fused"],
                      "launches_fused": launches(lambda: train(True)), "launches_plain": launches(lambda: train(False)),
                      "min_max_ms": spread, "routes": dict(routes)}))

    fresh = [[e.clone() for e in edges] for _ in range(32)]       # more pairs than the cache holds: every call is a miss
    turn = [0]

    def miss():
        turn[0] = (turn[0] + 1) % len(fresh)
        return infer(True, fresh[turn[0]])

    med, spread = alternate({"hit": lambda: infer(True), "miss": miss}, N, ROUNDS)
    print(json.dumps({"S": S, "leg": "edges", "hit_ms": med["hit"], "miss_ms": med["miss"], "miss_costs_ms": med["miss"] - med["hit"],
                      "launches_hit": launches(lambda: infer(True)), "launches_miss": launches(miss), "min_max_ms": spread}))

    os.environ["EQA_NBODY_KERNEL"] = "1"
    can = ea.EuclideanGroupNBody(net)
    nodes = torch.ones(M, 1, device=dev)
    w1, w2, w3 = torch.randn(M, 3, device=dev), torch.randn(M, 3, device=dev), torch.randn(M, 3, device=dev)

    def step(kernel):
        os.environ["EQA_NBODY_FRAME_KERNEL"] = "1" if kernel else "0"
        net.train()
        for p in net.parameters():
            p.grad = None
        cloc, cvel = can(nodes, loc=loc, edges=edges, vel=vel, edge_attr=None, charges=charges)
        back = can.invert_canonicalization(0.5 * cloc + cvel)
        routes["step fused" if kernel else "step plain"] = [net.last_route, can.last_route, can.last_invert_route]
        ((cloc * w1).sum() + (cvel * w2).sum() + (back * w3).sum()).backward()

    med, spread = alternate({"fused": lambda: step(True), "plain": lambda: step(False)}, N, ROUNDS)
    print(json.dumps({"S": S, "leg": "canonicalizer step", "fused_ms": med["fused"], "plain_ms": med["plain"],
                      "speedup": med["plain"] / med["fused"], "launches_fused": launches(lambda: step(True)),
                      "launches_plain": launches(lambda: step(False)), "min_max_ms": spread,
                      "routes": {k: v for k, v in routes.items() if k.startswith("step")}}))
os.environ.pop("EQA_NBODY_KERNEL", None)
os.environ.pop("EQA_NBODY_FRAME_KERNEL", None)
