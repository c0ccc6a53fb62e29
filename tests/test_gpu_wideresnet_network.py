"""WideResNet50Network / WideResNet101Network on the device: the fused eval route (every convolution behind the stem one call of
eqa_convwide_nhwc, batch-norms folded) against the plain route -- error budget, route and K-split tables, staleness of the folded
operands, what stays plain, graph capture, and the optimized canonicalizer end to end."""
import copy
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = ["conv1x1", "conv3x3", "conv1x1+res"]


def _routes(blocks):
    """Module order: the stem, then per block conv1, conv2, conv3 and downsample.0 where present."""
    out = ["lib"]
    for count in blocks:
        out += BLOCK + ["proj"] + BLOCK * (count - 1)
    return out


ROUTES50, ROUTES101 = _routes((3, 4, 6, 3)), _routes((3, 4, 23, 3))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _randomise_norms(net, seed):
    """Running statistics and affine parameters off the identity: identity statistics would hide a wrong fold.  (The spread is kept
    narrower than in the ResNet-18 test: 50 and 101 layers deep, a wider one overflows nothing but buries the head in one channel.)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.empty_like(m.weight).uniform_(0.7, 1.3, generator=g))
                m.bias.copy_(torch.empty_like(m.bias).normal_(0, 0.1, generator=g))
                m.running_mean.copy_(torch.empty_like(m.running_mean).normal_(0, 0.1, generator=g))
                m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.7, 1.3, generator=g))
    return net


def _net(dev, seed=11, cls="WideResNet50Network"):
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    return _randomise_norms(getattr(ea, cls)((3, 32, 32), 8, 3), seed + 1).to(dev).eval()


@pytest.fixture(scope="module")
def net50(dev):
    return _net(dev)


def _ref64(net, xs):
    """The plain route in fp64 on the CPU."""
    net64 = copy.deepcopy(net).double().cpu().eval()
    with torch.no_grad():
        return [net64.wideresnet(x.double().cpu()) for x in xs]


def _pooled(outs, refs):
    return sum(float((o.double().cpu() - r).pow(2).sum()) for o, r in zip(outs, refs)) ** 0.5


def _three_ways(net, xs, monkeypatch):
    """(fp64 reference, plain fp32 on the device, fused) outputs for the inputs xs, with the routes and splits each run reported."""
    refs = _ref64(net, xs)
    with torch.no_grad():
        monkeypatch.setenv("EQA_WIDERESNET_KERNEL", "0")
        plain = [net(x) for x in xs]
        routes_plain = list(net.last_routes)
        monkeypatch.delenv("EQA_WIDERESNET_KERNEL")
        fused = [net(x) for x in xs]
    return refs, plain, fused, routes_plain, list(net.last_routes), list(net.last_ksplits)


def _inputs(dev, seed=5):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(2, 3, 32, 32, device=dev, generator=g), torch.randn(3, 3, 40, 56, device=dev, generator=g)]


def _check_splits(routes, ksplits, n_layer4):
    assert len(ksplits) == len(routes) and ksplits[0] == 0
    for r, k in zip(routes, ksplits):
        assert (k == 0) if r == "lib" else (1 <= k <= 16), (r, k)
    assert all(k > 1 for k in ksplits[-n_layer4:]), ksplits[-n_layer4:]          # layer4: the longest K loops on the smallest maps


def test_fused_route_is_as_close_to_fp64_as_the_plain_route(dev, net50, monkeypatch):
    """B = 2 at 3 x 32 x 32 and B = 3 at 3 x 40 x 56 (stages 10 x 14, 5 x 7, 3 x 4, 2 x 2): the fused route's distance to the plain route in
    fp64 on the CPU, pooled 2-norm over the two cases, is at most 4 x the plain fp32 route's own on the device (the project's budget
    rule).  Measured at |out|_2 = 367: plain 2.8e-4, fused 2.1e-4."""
    xs = _inputs(dev)
    refs, plain, fused, routes_plain, routes_fused, ksplits = _three_ways(net50, xs, monkeypatch)
    assert routes_plain == ["plain"] * 53 and len(routes_fused) == 53
    for slot, (got, want) in enumerate(zip(routes_fused, ROUTES50)):
        assert got == want, (slot, got, want)
    _check_splits(routes_fused, ksplits, 10)
    assert fused[0].shape == (2, 128) and fused[1].shape == (3, 128) and all(bool(torch.isfinite(f).all()) for f in fused)
    d_plain, d_fused = _pooled(plain, refs), _pooled(fused, refs)
    scale = sum(float(r.pow(2).sum()) for r in refs) ** 0.5
    print(f"WideResNet50Network: |out|_2 = {scale:.3e}; to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}")
    assert d_fused <= 4 * d_plain, (d_fused, d_plain)


def test_the_101_runs_104_routes_inside_the_budget(dev, monkeypatch):
    """One B = 1 forward at 32 x 32.  Measured at |out|_2 = 1.36e4: plain 1.36e-2, fused 8.2e-3."""
    net = _net(dev, seed=17, cls="WideResNet101Network")
    xs = [torch.randn(1, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(8))]
    refs, plain, fused, routes_plain, routes_fused, ksplits = _three_ways(net, xs, monkeypatch)
    assert routes_plain == ["plain"] * 104 and routes_fused == ROUTES101
    _check_splits(routes_fused, ksplits, 10)
    d_plain, d_fused = _pooled(plain, refs), _pooled(fused, refs)
    scale = float(refs[0].norm())
    print(f"WideResNet101Network: |out|_2 = {scale:.3e}; to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}")
    assert fused[0].shape == (1, 128) and d_fused <= 4 * d_plain, (d_fused, d_plain)


def test_folded_operands_follow_every_change_of_their_sources(dev, monkeypatch):
    """An in-place write to one running_var, then an optimizer's write to one conv3.weight: each time the next fused output is within
    the budget of the NEW plain route, and the output from before the change is not."""
    net = _net(dev, seed=19)
    xs = _inputs(dev)[:1]

    def change_var(n):
        with torch.no_grad():
            n.wideresnet.layer3[2].bn2.running_var.mul_(4.0)

    def change_step(n):
        w = n.wideresnet.layer2[1].conv3.weight
        opt = torch.optim.SGD([w], lr=1.0)
        w.grad = 0.05 * torch.randn(w.shape, device=w.device, generator=torch.Generator(device=w.device).manual_seed(2))
        opt.step()
        w.grad = None

    with torch.no_grad():
        before = [net(x) for x in xs]
    assert net.last_routes == ROUTES50
    for change in (change_var, change_step):
        change(net)
        refs, plain, fused, _, routes_fused, _ = _three_ways(net, xs, monkeypatch)
        assert routes_fused == ROUTES50
        d_plain, d_fused, d_stale = _pooled(plain, refs), _pooled(fused, refs), _pooled(before, refs)
        print(f"{change.__name__}: to fp64: plain {d_plain:.3e}, fused {d_fused:.3e}, the output from before the change {d_stale:.3e}")
        assert not torch.equal(fused[0], before[0])
        assert d_fused <= 4 * d_plain, (change.__name__, d_fused, d_plain)
        assert d_stale > 4 * d_plain, (change.__name__, d_stale, d_plain)
        before = fused


def test_what_the_fused_rule_does_not_take_is_the_plain_route_bit_for_bit(dev, monkeypatch):
    """EQA_WIDERESNET_KERNEL=0, gradients enabled, the module in train(): the plain route, whose output is `net.wideresnet(x)` bit for
    bit -- compared with what `net.wideresnet` returned inside the very call (its forward is wrapped, which is no hook)."""
    net = _net(dev, seed=23)
    x = _inputs(dev)[0]
    seen = []
    inner = net.wideresnet.forward

    def recording(inp):
        seen.append((inp, inner(inp)))
        return seen[-1][1]

    monkeypatch.setattr(net.wideresnet, "forward", recording)

    def plain_and_equal():
        seen.clear()
        out = net(x)
        assert net.last_routes == ["plain"] * 53 and net.last_ksplits == [0] * 53 and len(seen) == 1 and seen[0][0] is x
        assert torch.equal(out, seen[0][1])
        return out

    with torch.no_grad():
        net(x)
        assert net.last_routes == ROUTES50 and not seen
        monkeypatch.setenv("EQA_WIDERESNET_KERNEL", "0")
        plain_and_equal()
        monkeypatch.delenv("EQA_WIDERESNET_KERNEL")
        monkeypatch.setenv("EQA_WRN_KERNEL", "0")                             # the ESCNN network's switch is not this one's
        seen.clear()
        net(x)
        assert net.last_routes == ROUTES50 and not seen
        monkeypatch.delenv("EQA_WRN_KERNEL")
    assert plain_and_equal().requires_grad                                  # gradients enabled
    with torch.no_grad():
        handle = net.wideresnet.layer2[0].conv2.register_forward_hook(lambda m, i, o: None)
        plain_and_equal()                                                   # a hook on a submodule the fused route would bypass
        handle.remove()
        net.train()
        mean_before = net.wideresnet.bn1.running_mean.clone()
        plain_and_equal()
        assert not torch.equal(net.wideresnet.bn1.running_mean, mean_before)    # (batch statistics: the modules ran as constructed)


def test_optimized_canonicalizer_end_to_end(dev, net50, monkeypatch):
    """OptimizedGroupEquivariantImageCanonicalization on the 50, D4 (roto-reflection, 4 rotations), resize_shape = 32, two 64 x 64 images:
    it canonicalizes and inverts, picks the same group element as with the switch off -- on a seed whose top-2 margins on the plain
    route are more than 100 x the largest fused - plain activation difference -- and the captured hipGraph of the step replays the
    eager fused step bit for bit."""
    import equiadapt_amd as ea
    from equiadapt_amd.graphs import GraphedCanonicalizer

    hp = types.SimpleNamespace(beta=1.0, input_crop_ratio=1.0, resize_shape=32, group_type="roto-reflection", num_rotations=4,
                               artifact_err_wt=0.0, learn_ref_vec=False)
    torch.manual_seed(31)
    can = ea.OptimizedGroupEquivariantImageCanonicalization(net50, hp, (3, 64, 64)).to(dev).eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(SEED)).to(dev)

    def run():
        with torch.no_grad():
            y = can(x)
            back = can.invert_canonicalization(y, induced_rep_type="scalar")
        info = can.canonicalization_info_dict
        return y, back, info["group_activations"].clone(), info["group_index"].clone(), list(net50.last_routes)

    monkeypatch.setenv("EQA_WIDERESNET_KERNEL", "0")
    y_p, b_p, a_p, g_p, r_p = run()
    monkeypatch.delenv("EQA_WIDERESNET_KERNEL")
    y_f, b_f, a_f, g_f, r_f = run()
    assert r_p == ["plain"] * 53 and r_f == ROUTES50
    assert y_f.shape == (2, 3, 64, 64) and b_f.shape == (2, 3, 64, 64) and a_f.shape == (2, 8)
    top2 = a_p.topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]).cpu()
    diff = (a_f - a_p).abs().max().item()
    print(f"activations: |fused - plain| <= {diff:.3e}; top-2 margins on the plain route {margin.tolist()}")
    assert bool((margin > 100 * diff).all()), (margin, diff)
    assert torch.equal(g_f, g_p)
    assert torch.equal(y_f, y_p) and torch.equal(b_f, b_p)
    assert bool(torch.isfinite(y_f).all()) and bool(torch.isfinite(b_f).all())
    step = GraphedCanonicalizer(can, x.shape)
    got = step(x)
    torch.cuda.synchronize()
    assert net50.last_routes == ROUTES50
    assert torch.equal(got[0], y_f) and torch.equal(got[1], g_f)


# of the canonicalizer test's images.  Measured on the MI355X over seeds 0 .. 9: seed 7 has top-2 margins 2.3e-4 and 7.2e-4 on the plain
# route against a largest fused - plain activation difference of 1.9e-7 (ratio 1200); seed 5's smaller margin is 9.8e-6 (ratio 76).
SEED = 7
