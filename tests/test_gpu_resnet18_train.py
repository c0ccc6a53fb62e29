"""ResNet18Network's opt-in training route (EQA_RESNET_TRAIN_KERNEL=1: Conv3x3Function + BnResActFunction on eqa_conv3x3_nhwc, its
two gradients and the eqa_bn_res_act_* family) against the plain route on the device and the plain route in fp64 on the CPU."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = ["conv3x3", "conv3x3+res"]
FUSED_ROUTES = ["lib"] + BLOCK * 2 + (BLOCK + ["conv1x1s2"] + BLOCK) * 3       # module order: conv1, conv2, downsample.0
TRAIN_ROUTES = ["lib:train"] + ["conv3x3:train"] * 4 + (["conv3x3:train"] * 2 + ["conv1x1s2:train"] + ["conv3x3:train"] * 2) * 3
KERNELS = ("conv3x3", "conv3x3_wgrad", "conv3x3_dgrad", "bn_res_act_fwd", "bn_res_act_bwd_reduce", "bn_res_act_bwd_apply")
SHAPES = [(4, 64, 64), (3, 40, 56)]          # every layer below 2048 pixels: nothing is gated


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _net(dev, seed=11):
    """Random weights, batch-norm weights, biases and running statistics off the identity (as test_gpu_resnet18_network.py's)."""
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    net = ea.ResNet18Network((3, 32, 32), 8, 3, out_vector_size=128)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.empty_like(m.weight).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty_like(m.bias).normal_(0, 0.1, generator=g))
                m.running_mean.copy_(torch.empty_like(m.running_mean).normal_(0, 0.1, generator=g))
                m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
    return net.to(dev).train()


def _batch(dev, shape, seed=5):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape[0], 3, shape[1], shape[2], device=dev, generator=g), torch.randn(shape[0], 128, device=dev, generator=g)


def _step(net, x, wgt):
    """One forward + backward of loss = <out, wgt>; -> (out, {name: gradient})."""
    net.zero_grad(set_to_none=True)
    out = net(x)
    (out * wgt).sum().backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def _dist(a, b64):
    return float((a.double().cpu() - b64).norm())


@pytest.fixture(scope="module")
def three_ways(dev):
    """Per shape: the training step of one network on one batch with the switch on, plain on the device, and in fp64 on the CPU (the
    truth) -- computed once for the tests below."""
    import os

    from equiadapt_amd import ops

    runs = {}
    for shape in SHAPES:
        net = _net(dev)
        x, wgt = _batch(dev, shape)
        plain, truth = copy.deepcopy(net), copy.deepcopy(net).double().cpu().train()
        old = os.environ.pop("EQA_RESNET_TRAIN_KERNEL", None)
        try:
            out_p, grads_p = _step(plain, x, wgt)
            routes_p = list(plain.last_routes)
            os.environ["EQA_RESNET_TRAIN_KERNEL"] = "1"
            with ops.KernelTimer() as timer:
                out_k, grads_k = _step(net, x, wgt)
            seen = timer.summary()
        finally:
            os.environ.pop("EQA_RESNET_TRAIN_KERNEL", None)
            if old is not None:
                os.environ["EQA_RESNET_TRAIN_KERNEL"] = old
        out_t, grads_t = _step(truth, x.double().cpu(), wgt.double().cpu())
        runs[shape] = dict(net=net, plain=plain, truth=truth, routes_p=routes_p, seen=seen, outs=(out_k, out_p, out_t),
                           grads=(grads_k, grads_p, grads_t))
    return runs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_training_step_is_as_close_to_fp64_as_the_plain_route(three_ways, shape):
    """Output and every one of the 62 parameter gradients: the kernel route's distance (2-norm) to the fp64 truth is at most 4 x the
    plain fp32 route's own -- the budget of test_gpu_resnet18_network.py.  Route tables, the launches seen, the running statistics.
    Measured on the MI355X: see the printed ratios (DESIGN.md section 1 records them)."""
    r = three_ways[shape]
    net, truth = r["net"], r["truth"]
    assert r["routes_p"] == ["plain"] * 20
    assert net.last_routes == TRAIN_ROUTES, net.last_routes
    assert net.last_wgrad_routes == ["lib"] + ["kernel"] * 19, net.last_wgrad_routes
    for name in KERNELS:
        assert name in r["seen"] and r["seen"][name][0] >= 1, (name, sorted(r["seen"]))
    (out_k, out_p, out_t), (grads_k, grads_p, grads_t) = r["outs"], r["grads"]
    assert len(grads_k) == 62 and all(bool(torch.isfinite(g).all()) for g in grads_k.values())
    d_k, d_p = _dist(out_k, out_t), _dist(out_p, out_t)
    print(f"{shape}: output |.|_2 = {float(out_t.norm()):.3e}; to fp64: plain {d_p:.3e}, kernels {d_k:.3e} (ratio {d_k / max(d_p, 1e-300):.2f})")
    worst = ("", 0.0)
    failed = []
    for name in grads_t:
        g_k, g_p = _dist(grads_k[name], grads_t[name]), _dist(grads_p[name], grads_t[name])
        ratio = g_k / g_p if g_p > 0 else (0.0 if g_k == 0 else float("inf"))
        print(f"  {name}: |g|_2 = {float(grads_t[name].norm()):.3e}; plain {g_p:.3e}, kernels {g_k:.3e} (ratio {ratio:.2f})")
        worst = max(worst, (name, ratio), key=lambda t: t[1])
        if g_k > 4 * g_p:
            failed.append((name, g_k, g_p))
    print(f"{shape}: worst gradient ratio {worst[1]:.2f} at {worst[0]}")
    assert d_k <= 4 * d_p, (d_k, d_p)
    assert not failed, failed
    for (name, b), (_, b_t) in zip(net.named_buffers(), truth.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(b) == 1, name
        else:
            assert torch.allclose(b.double().cpu(), b_t, atol=1e-5, rtol=1e-4), name


def test_the_route_is_opt_in_and_what_its_rule_does_not_take_runs_plain(dev, monkeypatch):
    """Switch unset: training runs `net.resnet18(x)` once, as the committed suite pins it.  Switch on with one batch-norm in eval(), a
    forward hook on a submodule, EQA_RESNET_KERNEL=0, or an fp64 network and input: plain as well."""
    net = _net(dev)
    x, _ = _batch(dev, (2, 32, 32))
    calls = []

    def record(n):
        inner = n.resnet18.forward

        def recording(inp):
            calls.append(inp)
            return inner(inp)

        monkeypatch.setattr(n.resnet18, "forward", recording)

    net64 = copy.deepcopy(net).double()
    record(net)
    record(net64)

    def runs_plain(n=net, inp=x):
        calls.clear()
        out = n(inp)
        assert n.last_routes == ["plain"] * 20 and n.last_wgrad_routes == [] and len(calls) == 1 and calls[0] is inp
        return out

    monkeypatch.delenv("EQA_RESNET_TRAIN_KERNEL", raising=False)
    assert runs_plain().requires_grad
    monkeypatch.setenv("EQA_RESNET_TRAIN_KERNEL", "0")
    runs_plain()
    monkeypatch.setenv("EQA_RESNET_TRAIN_KERNEL", "1")
    calls.clear()
    assert net(x).requires_grad and net.last_routes == TRAIN_ROUTES and not calls
    net.resnet18.layer3[1].bn2.eval()
    runs_plain()
    net.resnet18.layer3[1].bn2.train()
    handle = net.resnet18.layer2[0].conv2.register_forward_hook(lambda m, i, o: None)
    runs_plain()
    handle.remove()
    monkeypatch.setenv("EQA_RESNET_KERNEL", "0")
    runs_plain()
    monkeypatch.delenv("EQA_RESNET_KERNEL")
    runs_plain(net64, x.double())
    calls.clear()
    net(x)
    assert net.last_routes == TRAIN_ROUTES and not calls


def test_a_kernel_route_step_reaches_the_eval_routes_cache(dev, monkeypatch):
    """The running statistics written by eqa_bn_act_finalize, then the stepped weights: after each, the next eval forward under
    no_grad is the fused route and within 4 x the plain route's distance to fp64 of the NEW plain route, while the fused output cached
    before is not."""
    net = _net(dev)
    x, wgt = _batch(dev, (4, 32, 32), seed=3)
    opt = torch.optim.SGD(net.parameters(), lr=1e-4)      # (gradients of norm 1e2 .. 1e3 against weights of norm ~ 10: a step that stays finite)

    def eval_three_ways():
        net.eval()
        net64 = copy.deepcopy(net).double().cpu().eval()
        with torch.no_grad():
            ref = net64.resnet18(x.double().cpu())
            monkeypatch.setenv("EQA_RESNET_KERNEL", "0")
            plain = net(x)
            monkeypatch.delenv("EQA_RESNET_KERNEL")
            fused = net(x)
        assert net.last_routes == FUSED_ROUTES
        net.train()
        return ref, plain, fused

    monkeypatch.setenv("EQA_RESNET_TRAIN_KERNEL", "1")
    _, _, before = eval_three_ways()
    _step(net, x, wgt)
    assert net.last_routes == TRAIN_ROUTES
    for what in ("running statistics", "weights"):
        if what == "weights":
            opt.step()
        ref, plain, fused = eval_three_ways()
        d_plain, d_fused, d_stale = _dist(plain, ref), _dist(fused, ref), _dist(before, ref)
        print(f"after the {what} changed: to fp64: plain {d_plain:.3e}, fused {d_fused:.3e}, the output from before {d_stale:.3e}")
        assert d_fused <= 4 * d_plain and d_stale > 4 * d_plain, (what, d_fused, d_plain, d_stale)
        before = fused


def test_layers_the_gate_hands_to_the_library_stay_inside_the_budget(dev, monkeypatch):
    """`_kernel_pays` refusing stages 3 and 4: their ten layers run the library's convolution under autograd ("lib:train", the batch-norm
    block still on the kernels), the rest stay; the same budget holds for the output and every gradient."""
    shape = SHAPES[0]
    net = _net(dev)
    x, wgt = _batch(dev, shape)
    plain, truth = copy.deepcopy(net), copy.deepcopy(net).double().cpu().train()
    monkeypatch.delenv("EQA_RESNET_TRAIN_KERNEL", raising=False)
    out_p, grads_p = _step(plain, x, wgt)
    out_t, grads_t = _step(truth, x.double().cpu(), wgt.double().cpu())
    monkeypatch.setenv("EQA_RESNET_TRAIN_KERNEL", "1")
    monkeypatch.setattr(net, "_kernel_pays", lambda pixels, cin, taps, stride: not (cin >= 256 or (cin == 128 and stride == 2)), raising=False)
    out_k, grads_k = _step(net, x, wgt)
    assert net.last_routes == TRAIN_ROUTES[:10] + ["lib:train"] * 10, net.last_routes
    assert net.last_wgrad_routes == ["lib"] + ["kernel"] * 9 + ["lib"] * 10
    d_k, d_p = _dist(out_k, out_t), _dist(out_p, out_t)
    print(f"gated: output to fp64: plain {d_p:.3e}, kernels {d_k:.3e}")
    assert d_k <= 4 * d_p, (d_k, d_p)
    failed = []
    for name in grads_t:
        g_k, g_p = _dist(grads_k[name], grads_t[name]), _dist(grads_p[name], grads_t[name])
        print(f"  {name}: plain {g_p:.3e}, kernels {g_k:.3e}")
        if g_k > 4 * g_p:
            failed.append((name, g_k, g_p))
    assert not failed, failed


def test_two_steps_on_one_batch_give_the_same_bits_on_the_kernel_layers(dev, monkeypatch):
    """Same weights, same batch, twice: every gradient behind the stem is bit-equal (no atomics on the kernel route); the stem's own
    gradients come from the library and are excluded."""
    monkeypatch.setenv("EQA_RESNET_TRAIN_KERNEL", "1")
    net = _net(dev)
    x, wgt = _batch(dev, SHAPES[1])
    a_out, a = _step(copy.deepcopy(net), x, wgt)
    b_out, b = _step(copy.deepcopy(net), x, wgt)
    assert torch.equal(a_out, b_out)
    for name in a:
        if not (name.startswith("resnet18.conv1.") or name.startswith("resnet18.bn1.")):
            assert torch.equal(a[name], b[name]), name
