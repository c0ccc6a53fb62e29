"""The 16-multiple channel contractions alone, and the steerable.yaml network's eval forward and training step with and without them:
python tools/kbench_cgemm3m_c16.py [--small] [--net-only] [--kernels-only] [M,Cin,Cout ...]

1. Per shape (M tiles, Cin, Cout) -- (1024, 144, 144): the configuration's hidden layers at B = 256; (72, 144, 144); (1024, 48, 80);
   (1024, 288, 288) -- alternating, back to back:
     c16 / lib              eqa_fft48_cgemm3m_c16 against torch.bmm on the real (F, 2Cin, 2Cout) form (what EQA_FFT_GEMM_C16=0 runs)
     wgrad_c16 / wgrad_lib  eqa_fft48_wgrad3m_c16 against torch.bmm(V^T, G)
   Effective TFLOP/s on 1154 M Cin Cout 8 (the flops of the four-product form, whichever form ran).  `admitted`: the new kernel's
   median is below the library's by more than the larger of the two min-max spreads.
2. ESCNNSteerableNetwork((3, 96, 96), 16 fields, k = 7, 3 layers) at B = 256: eval forward under no_grad and training step
   (forward + backward of (out * w).sum()), fftconv.GEMM_C16 on against off, alternating (two copies of the network: in eval each
   keeps the filter operand of its own route).
One JSON line per measurement: medians of 5 x 20 (kernels) / 5 x 3 (network) with the (min, max) of the rounds.  --small: toy sizes,
to rehearse the script."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import equiadapt_amd as ea
from equiadapt_amd import _lib, ops
from equiadapt_amd.images.canonicalization_networks import fftconv

dev = torch.device("cuda:0")
small = "--small" in sys.argv
NF = fftconv.F


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


def admitted(med, spread, new, old):
    margin = max(spread[new][1] - spread[new][0], spread[old][1] - spread[old][0])
    return med[new] < med[old] - margin


def contraction(M, cin, cout):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    bank = torch.randn(cout, cin, 7, 7, device=dev) / (cin * 49) ** 0.5
    sp = fftconv.filter_spectra3m_c16(bank)
    real = torch.empty((NF, 2 * cin, 2 * cout), dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_fft48_filter_spectra(bank.data_ptr(), real.data_ptr(), cout, cin, 7, 1, st), "eqa_fft48_filter_spectra")
    V = fftconv.spectra_buffer(M, 2 * cin, dev).normal_()
    G = fftconv.spectra_buffer(M, 2 * cout, dev).normal_()
    mo_c16, mo_lib = fftconv.spectra_buffer(M, 2 * cout, dev), fftconv.spectra_buffer(M, 2 * cout, dev)
    d3 = torch.empty((NF, cin, 2, cout), dtype=torch.float32, device=dev)

    def c16():
        _lib.check(lib.eqa_fft48_cgemm3m_c16(V.data_ptr(), sp.data.data_ptr(), mo_c16.data_ptr(), M, cin, cout, st), "eqa_fft48_cgemm3m_c16")

    def wgrad_c16():
        _lib.check(lib.eqa_fft48_wgrad3m_c16(V.data_ptr(), G.data_ptr(), d3.data_ptr(), M, cin, cout, st), "eqa_fft48_wgrad3m_c16")

    c16()
    torch.bmm(V, real, out=mo_lib)
    err = float((mo_c16 - mo_lib).abs().max() / mo_lib.abs().max())
    wgrad_c16()
    dl = torch.bmm(V.transpose(1, 2), G)                             # (F, 2Cin, 2Cout): rows [Re x 16 | Im x 16], columns likewise
    ci, co = torch.arange(cin, device=dev), torch.arange(cout, device=dev)
    rr, ri = (ci // 16) * 32 + ci % 16, (ci // 16) * 32 + 16 + ci % 16
    cr, cim = (co // 16) * 32 + co % 16, (co // 16) * 32 + 16 + co % 16
    dr = dl[:, rr][:, :, cr] + dl[:, ri][:, :, cim]
    di = dl[:, ri][:, :, cr] - dl[:, rr][:, :, cim]
    werr = float(max((d3[:, :, 0] - dr).abs().max() / dr.abs().max(), (d3[:, :, 1] - di).abs().max() / di.abs().max()))
    del dl, dr, di
    med, spread = alternate({"c16": c16, "lib": lambda: torch.bmm(V, real, out=mo_lib),
                             "wgrad_c16": wgrad_c16, "wgrad_lib": lambda: torch.bmm(V.transpose(1, 2), G)}, n=20, rounds=5)
    flop = NF * M * cin * cout * 8.0
    print(json.dumps({"what": "cgemm3m_c16 kernels", "M": M, "Cin": cin, "Cout": cout, "median_ms": med, "min_max_ms": spread,
                      "effective_TFLOPs": {k: flop / v / 1e9 for k, v in med.items()},
                      "speedup_over_lib": med["lib"] / med["c16"], "wgrad_speedup_over_lib": med["wgrad_lib"] / med["wgrad_c16"],
                      "admitted": admitted(med, spread, "c16", "lib"), "wgrad_admitted": admitted(med, spread, "wgrad_c16", "wgrad_lib"),
                      "rel_diff": err, "rel_diff_wgrad": werr}), flush=True)


shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:] if a[0].isdigit()]          # M,Cin,Cout ...: these instead
if "--net-only" not in sys.argv:
    for shape in shapes or ([(40, 48, 80), (9, 144, 144)] if small else [(1024, 144, 144), (72, 144, 144), (1024, 48, 80), (1024, 288, 288)]):
        contraction(*shape)
        torch.cuda.empty_cache()
if "--kernels-only" in sys.argv:
    sys.exit(0)

B, hw = (2, 64) if small else (256, 96)
torch.manual_seed(0)
nets = {True: ea.ESCNNSteerableNetwork((3, hw, hw), 16, 7, "rotation", 3).to(dev)}
nets[False] = copy.deepcopy(nets[True])
img = torch.randn(B, 3, hw, hw, device=dev)
w = torch.randn(B, 2, 2, device=dev)


def forward(on):
    fftconv.GEMM_C16 = on
    with torch.no_grad():
        return nets[on](img)


def step(on):
    fftconv.GEMM_C16 = on
    nets[on].zero_grad(set_to_none=True)
    out = nets[on](img)
    (out * w).sum().backward()
    return out.detach()


def launches(fn):
    got = {}
    for on in (True, False):
        with ops.KernelTimer() as t:
            fn(on)
        got["on" if on else "off"] = {"routes": list(nets[on].last_routes), "contraction": fftconv.LAST_CONTRACTION, "wgrad": fftconv.LAST_WGRAD,
                                      **{k: [v[0], round(v[1], 4)] for k, v in t.summary().items()}}
    return got


for net in nets.values():
    net.eval()
ref, got = forward(False), forward(True)
err = float((got - ref).abs().max() / ref.abs().max())
med, spread = alternate({"on": lambda: forward(True), "off": lambda: forward(False)}, n=3, rounds=5)
print(json.dumps({"what": "steerable.yaml network eval forward", "B": B, "hw": hw, "on_ms": med["on"], "off_ms": med["off"],
                  "speedup": med["off"] / med["on"], "rel_diff_of_outputs": err, "min_max_ms": spread,
                  "library_launches_count_mean_ms": launches(forward)}), flush=True)

for net in nets.values():
    net.train()
ref, got = step(False), step(True)
err = float((got - ref).abs().max() / ref.abs().max())
gerr = max(float((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30))
           for p, q in zip(nets[True].parameters(), nets[False].parameters()))
med, spread = alternate({"on": lambda: step(True), "off": lambda: step(False)}, n=3, rounds=5)
print(json.dumps({"what": "steerable.yaml network training step", "B": B, "hw": hw, "on_ms": med["on"], "off_ms": med["off"],
                  "speedup": med["off"] / med["on"], "rel_diff_of_outputs": err, "rel_diff_of_gradients": gerr, "min_max_ms": spread,
                  "library_launches_count_mean_ms": launches(step)}), flush=True)
fftconv.GEMM_C16 = True
