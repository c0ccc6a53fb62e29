"""ESCNNWRNEquivariantNetwork's training route (wrn_networks._forward_training: GConv1x1Function, the convolution Functions, the fused
batch-norm kernels, window sums) against the plain route in fp64: one forward + backward from the same state through the training
route in fp32, the plain route in fp32 (EQA_WRN_KERNEL=0) and the plain route in fp64 on the device.

The budget is the project's standing one for a fused route: 4 x the plain fp32 route's own distance to fp64 -- pooled over all
parameter gradients; per parameter with that parameter's own plain error, floored at the pooled per-element rms plain error x
sqrt(numel) (an exactly cancelling gradient, such as that of a bias in front of a batch-norm with batch statistics, has no plain
error to speak of); for the output; for every running_mean / running_var.

A gradient can be compared across precisions only where the network is differentiable within the precision's reach: a ReLU input that
is 1e-8 in fp64 is on either side of zero in fp32, by the summation order of whatever convolution algorithm the library picked, and
one such element moves the pooled gradient by 1e-3 of its norm.  With 1.5 (C4) to 3 (D4) million ReLU inputs of unit scale, a random
state has some within 1e-6 of zero.  So the state is chosen where there are none (`_keep_relu_inputs_off_zero`): the test randomises
the batch-norm biases anyway, and each field's bias is moved, by at most 2e-2 (they are drawn with a deviation of 0.1), to the middle of the widest gap that its fp64 ReLU
inputs leave near zero.  The margin asked for, 1e-4 = 1700 x 2^-24 of the rms value of the field's ReLU inputs (rounding is
relative to the values' scale, and with running statistics a field's scale can be a tenth of another's), is an order above the rounding
fp32 accumulates through the network's 17 convolutions of up to 4608 terms; it is verified on the fp64 reference of the state used."""
import copy
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _net(dev, group, out_channels, in_shape=(3, 33, 33), k=3, layers=6, seed=11):
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    net = ea.ESCNNWRNEquivariantNetwork(in_shape, out_channels, k, group, layers, 4)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "expanded_weights"):
                m.bias.normal_(0, 0.1)
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return net.to(dev)


def _one_by_ones(net):
    """Positions in last_routes of the bottlenecks' 1 x 1 convolutions (first, second)."""
    import equiadapt_amd as ea

    pos, at = [], 1                                               # (0: the stem)
    for m in net.eqv_network:
        if isinstance(m, ea.ESCNNWideBottleneck):
            pos.append((at, at + 2))
        if isinstance(m, (ea.ESCNNWideBottleneck, ea.ESCNNWideBasic)):
            at += 3
    return pos


class _env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("EQA_WRN_KERNEL")
        os.environ["EQA_WRN_KERNEL"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("EQA_WRN_KERNEL", None)
        else:
            os.environ["EQA_WRN_KERNEL"] = self.old


def _step(net, x, wgt):
    """One forward + backward of a copy of net: output, gradients, buffers, routes (all as fp64 where they are numbers)."""
    net = copy.deepcopy(net).to(x.dtype)
    out = net(x)
    (out.double() * wgt).sum().backward()
    return types.SimpleNamespace(
        out=out.detach().double(), routes=list(net.last_routes),
        grads={n: (None if p.grad is None else p.grad.double()) for n, p in net.named_parameters()},
        stats={n: b.detach().double() for n, b in net.named_buffers() if not n.endswith("num_batches_tracked")},
        counts={n: int(b) for n, b in net.named_buffers() if n.endswith("num_batches_tracked")})


MARGIN = 1e-4        # no fp64 ReLU input of the reference may be closer to zero, as a fraction of its field's rms value (module docstring)
REACH = 2e-2         # how far a field's batch-norm bias may move for it


def _relu_inputs_pass(net, x, move):
    """One plain fp64 forward of a copy of net (in net's mode).  Every batch-norm output -- the input of the ReLU behind it -- is seen
    on the way; with `move`, each field's output is shifted so that zero lies in the middle of the widest gap between neighbouring
    values within REACH of it, and what follows sees the shifted map.  Returns ({batch-norm name: shift per field}, the smallest
    distance of any ReLU input to zero as a fraction of the rms value of its field's inputs)."""
    net64 = copy.deepcopy(net).double()
    shifts, closest = {}, [float("inf")]

    def hook(name):
        def fn(mod, inp, out):
            fields = out.shape[1]
            if move:
                ys = out.detach().transpose(0, 1).reshape(fields, -1)
                # (two sentinels at -2 REACH and 2 REACH: a field with fewer than two values near zero -- running statistics can put all
                # of it on one side -- has the gaps next to them to choose from, and an empty neighbourhood of zero gives shift 0)
                ends = ys.new_tensor([-2 * REACH, 2 * REACH]).expand(fields, 2)
                ys = torch.cat([ys, ends], dim=1).sort(dim=1).values
                mid, gap = (ys[:, 1:] + ys[:, :-1]) / 2, ys[:, 1:] - ys[:, :-1]
                j = torch.where(mid.abs() <= REACH, gap, torch.zeros_like(gap)).argmax(dim=1, keepdim=True)
                delta = -mid.gather(1, j)[:, 0]
                shifts[name] = delta
                out = out + delta[None, :, None, None, None]
            yf = out.detach().transpose(0, 1).reshape(fields, -1)
            closest[0] = min(closest[0], float((yf.abs().min(dim=1).values / yf.pow(2).mean(dim=1).sqrt()).min()))
            return out
        return fn

    for name, m in net64.named_modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.register_forward_hook(hook(name))
    with torch.no_grad():
        net64(x.double())
    assert set(net64.last_routes) == {"conv2d"}
    return shifts, closest[0]


def _keep_relu_inputs_off_zero(net, x):
    """Move net's batch-norm biases (in place) so that no ReLU input of its plain fp64 evaluation at x is within MARGIN of zero, and
    verify that on a second evaluation of the moved state.  Returns the margin found."""
    shifts, _ = _relu_inputs_pass(net, x, move=True)
    mods = dict(net.named_modules())
    with torch.no_grad():
        for name, delta in shifts.items():
            assert float(delta.abs().max()) <= REACH
            mods[name].bias += delta.to(mods[name].bias.dtype)
    _, closest = _relu_inputs_pass(net, x, move=False)
    assert closest >= MARGIN, closest
    return closest


_RUNS = {}


def _runs(dev, group, frozen=False):
    """The three steps of one configuration ((3, 33, 33), out_channels = 32, k = 3, 6 layers, B = 2), shared by the tests below."""
    key = (group, frozen)
    if key in _RUNS:
        return _RUNS[key]
    net = _net(dev, group, 32)
    net = net.eval() if frozen else net.train()
    x = torch.randn(2, 3, 33, 33, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    closest = _keep_relu_inputs_off_zero(net, x)
    print(f"{group}{', frozen batch-norm' if frozen else ''}: closest fp64 ReLU input to zero {closest:.3e} of its field's rms")
    wgt = torch.randn(2, 4 if group == "rotation" else 8, device=dev, generator=torch.Generator(device=dev).manual_seed(6)).double()
    before = {n: b.detach().clone() for n, b in net.named_buffers()}
    with _env("1"):
        fused = _step(net, x, wgt)
    with _env("0"):
        plain = _step(net, x, wgt)
    ref = _step(net, x.double(), wgt)
    _RUNS[key] = types.SimpleNamespace(net=net, fused=fused, plain=plain, ref=ref, before=before)
    return _RUNS[key]


def _norm(t):
    return float(t.norm())


def _hold_to_the_budget(r, tag):
    names = list(r.ref.grads)
    assert all(r.fused.grads[n] is not None for n in names), [n for n in names if r.fused.grads[n] is None]
    d_f = {n: _norm(r.fused.grads[n] - r.ref.grads[n]) for n in names}
    d_p = {n: _norm(r.plain.grads[n] - r.ref.grads[n]) for n in names}
    numel = {n: r.ref.grads[n].numel() for n in names}
    pooled_f, pooled_p = sum(v * v for v in d_f.values()) ** 0.5, sum(v * v for v in d_p.values()) ** 0.5
    pooled_ref = sum(_norm(r.ref.grads[n]) ** 2 for n in names) ** 0.5
    rms_p = pooled_p / sum(numel.values()) ** 0.5
    o_f, o_p = _norm(r.fused.out - r.ref.out), _norm(r.plain.out - r.ref.out)
    print(f"{tag}: |grad| {pooled_ref:.3e}; to fp64, pooled over the gradients: plain fp32 {pooled_p:.3e}, training route {pooled_f:.3e}; "
          f"output (|out| {_norm(r.ref.out):.3e}): plain {o_p:.3e}, training route {o_f:.3e}")
    worst = max(names, key=lambda n: d_f[n] / max(d_p[n], rms_p * numel[n] ** 0.5))
    print(f"{tag}: worst parameter {worst}: training route {d_f[worst]:.3e}, plain {d_p[worst]:.3e}, floor {rms_p * numel[worst] ** 0.5:.3e}")
    s_f = {n: _norm(r.fused.stats[n] - r.ref.stats[n]) for n in r.ref.stats}
    s_p = {n: _norm(r.plain.stats[n] - r.ref.stats[n]) for n in r.ref.stats}
    worst_s = max(s_f, key=lambda n: s_f[n] / max(s_p[n], 1e-300))
    print(f"{tag}: worst running statistic {worst_s}: training route {s_f[worst_s]:.3e}, plain {s_p[worst_s]:.3e}")
    assert pooled_f <= 4 * pooled_p, (pooled_f, pooled_p)
    for n in names:
        assert d_f[n] <= 4 * max(d_p[n], rms_p * numel[n] ** 0.5), (n, d_f[n], d_p[n], rms_p * numel[n] ** 0.5)
    assert o_f <= 4 * o_p, (o_f, o_p)
    for n in s_f:
        assert s_f[n] <= 4 * s_p[n], (n, s_f[n], s_p[n])
    assert r.fused.counts == r.ref.counts == r.plain.counts


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_training_route_is_as_close_to_fp64_as_the_plain_route(dev, group):
    """train(): batch statistics, running statistics updated.  The budget of the module docstring; figures in DESIGN.md."""
    r = _runs(dev, group)
    assert all(v == 1 for v in r.ref.counts.values())
    some = next(n for n in r.ref.stats if n.endswith("running_mean"))
    assert (r.fused.stats[some] - r.before[some].double()).abs().max().item() > 1e-4          # momentum 0.9: it moved
    _hold_to_the_budget(r, group)


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_routes(dev, group):
    """The training route names its kernels; EQA_WRN_KERNEL=0 and fp64 run the plain route."""
    r = _runs(dev, group)
    routes = r.fused.routes
    assert len(routes) == 17 and "conv2d" not in routes, routes
    for first, second in _one_by_ones(r.net):
        assert (routes[first], routes[second]) == ("gconv1x1", "gconv1x1+junction"), routes
    assert routes[0] in ("lift", "lift_wide") and routes[-1] == "window_sums", routes
    assert set(r.plain.routes) == {"conv2d"} and set(r.ref.routes) == {"conv2d"} and len(r.plain.routes) == 17


def test_narrow_networks_and_networks_without_bottlenecks(dev):
    """The entry rule asks for one bottleneck 1 x 1 layer that the kernels take.  num_layers = 3 has no bottleneck, out_channels = 4
    has them at 4, 8 and 16 channels, all below the gate of 32: the plain route, as before.  out_channels = 8 (C4: 8, 16 and 32
    channels) has its last bottleneck on the gate: that one runs on the kernels, the narrow ones on the library's convolution
    inside the training route."""
    x = torch.randn(2, 3, 33, 33, device=dev)
    for kwargs in ({"out_channels": 8, "layers": 3}, {"out_channels": 4}):
        net = _net(dev, "rotation", **kwargs).train()
        net(x).sum().backward()
        assert set(net.last_routes) == {"conv2d"}, (kwargs, net.last_routes)
        assert all(p.grad is not None for p in net.parameters())
    net = _net(dev, "rotation", 8).train()
    net(x).sum().backward()
    ones = [net.last_routes[i] for pair in _one_by_ones(net) for i in pair]
    assert ones == ["lib", "lib", "lib", "lib", "gconv1x1", "gconv1x1+junction"] and "conv2d" not in net.last_routes, net.last_routes
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_frozen_batch_norm(dev, group):
    """eval() with gradients enabled: the running statistics are used and left as they were; same budget."""
    r = _runs(dev, group, frozen=True)
    assert "conv2d" not in r.fused.routes and "gconv1x1+junction" in r.fused.routes
    for n, b in r.before.items():
        after = r.fused.counts[n] if n.endswith("num_batches_tracked") else r.fused.stats[n]
        assert (int(b) == after) if n.endswith("num_batches_tracked") else torch.equal(b.double(), after), n
    _hold_to_the_budget(r, f"{group}, frozen batch-norm")
    live = _runs(dev, group)
    assert (live.ref.out - r.ref.out).abs().max().item() > 1e-6, "batch and running statistics must give different outputs"


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_every_parameter_has_a_finite_gradient(dev, group):
    r = _runs(dev, group)
    for n, g in r.fused.grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), n
    assert sum(float(g.abs().sum()) > 0 for g in r.fused.grads.values()) > len(r.fused.grads) // 2
