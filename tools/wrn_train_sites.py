"""Where ESCNNWRNEquivariantNetwork's training route stops being reproducible bit for bit, and what that does to its gradients:
python tools/wrn_train_sites.py [--after-c4] [--off-zero]

The D4 network of tests/test_gpu_wrn_train.py ((3, 33, 33), out_channels = 32, k = 3, 6 layers, B = 2, train()) in its raw random state
(--off-zero: in the state the test uses, every fp64 ReLU input at least 1e-4 of its field's rms value from zero).  Two steps through the training route, one
through the plain route in fp64 and in fp32; then, per batch-norm + ReLU site in call order: a bit checksum of the training route's
input and output, whether the two steps of this process gave the same bits, the distance of the site's input to fp64 (sites behind a
k x k layer differ by that layer's bias, which the training route hands to the batch-norm), and the ReLU inputs of the fp64 route at
every element whose mask differs.  Last: the library's convolution twice on the same channels-last operands at the shapes of the first
WideBasic block.  --after-c4: run the test file's C4 case first in the process."""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch

import test_gpu_wrn_train as T
from equiadapt_amd.images.canonicalization_networks import wrn_networks as W

dev = torch.device("cuda:0")
if "--after-c4" in sys.argv:
    T._runs(dev, "rotation")
group = "roto-reflection"
net0 = T._net(dev, group, 32).train()
x = torch.randn(2, 3, 33, 33, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
if "--off-zero" in sys.argv:
    print("closest fp64 ReLU input to zero: %.3e" % T._keep_relu_inputs_off_zero(net0, x))
wgt = torch.randn(2, 8, device=dev, generator=torch.Generator(device=dev).manual_seed(6)).double()

rec = []
real = W.InnerBnReluDropout


class Spy:
    @staticmethod
    def apply(h, *a):
        y = real.apply(h, *a)
        rec.append((h.detach().clone(), y.detach().clone()))
        return y


def train_run():
    rec.clear()
    W.InnerBnReluDropout = Spy
    os.environ["EQA_WRN_KERNEL"] = "1"
    try:
        r = T._step(net0, x, wgt)
    finally:
        W.InnerBnReluDropout = real
    return r, list(rec)


def module_run(dtype):
    os.environ["EQA_WRN_KERNEL"] = "0"
    net = copy.deepcopy(net0).to(dtype)
    pre = []
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.register_forward_hook(lambda mod, i, o: pre.append((i[0].detach().flatten(1, 2).clone(), o.detach().flatten(1, 2).clone())))
    out = net(x.to(dtype))
    (out.double() * wgt).sum().backward()
    return {n: p.grad.double() for n, p in net.named_parameters()}, pre


def cs(t):
    return int(t.contiguous().view(torch.int32).sum(dtype=torch.int64))


r1, t1 = train_run()
r2, t2 = train_run()
g64, p64 = module_run(torch.float64)
g32, p32 = module_run(torch.float32)
names = list(g64)
print("pooled: train-ref %.3e plain-ref %.3e train-plain %.3e train-train %.3e" % tuple(
    sum(float((a[n] - b[n]).norm()) ** 2 for n in names) ** 0.5
    for a, b in ((r1.grads, g64), (g32, g64), (r1.grads, g32), (r1.grads, r2.grads))))
for i, ((h, y), (h2, y2), (i64, o64), (i32, o32)) in enumerate(zip(t1, t2, p64, p32)):
    ft = (y > 0) != (o64 > 0)
    fp = (o32 > 0) != (o64 > 0)
    print(f"site {i:2d} C={y.shape[1]:3d} in-cs {cs(h):14d} out-cs {cs(y):14d} same-in-process {cs(h) == cs(h2) and cs(y) == cs(y2)} "
          f"|h-h64| {float((h.double() - i64).abs().max()):.2e} plain |h-h64| {float((i32.double() - i64).abs().max()):.2e} "
          f"flips train {int(ft.sum())} {[f'{v:.1e}' for v in o64[ft].tolist()][:4]} plain {int(fp.sum())} {[f'{v:.1e}' for v in o64[fp].tolist()][:4]}")

import torch.nn.functional as F

NHWC = torch.channels_last
for cin, cout, k, H in ((64, 128, 3, 31), (128, 128, 3, 29), (64, 128, 5, 31)):
    torch.manual_seed(0)
    xx = torch.randn(2, cin, H, H, device=dev).contiguous(memory_format=NHWC).requires_grad_()
    ww = (torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5).contiguous(memory_format=NHWC).requires_grad_()
    got = []
    for _ in range(3):
        xx.grad = ww.grad = None
        y = F.conv2d(xx, ww)
        y.backward(torch.ones_like(y) * 0.5 + y.detach())
        got.append((cs(y.detach()), cs(xx.grad), cs(ww.grad)))
    print(f"F.conv2d {cin}->{cout} k={k} at {H}x{H}, channels-last, three calls: same bits (y, dx, dw):",
          [len({g[i] for g in got}) == 1 for i in range(3)])
