"""ResNet18Network on the device: the fused eval route (19 of 20 convolutions on eqa_conv3x3_nhwc, batch-norms folded) against the
plain route -- error budget, route table, staleness of the folded operands, training, and the optimized canonicalizer end to end."""
import copy
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = ["conv3x3", "conv3x3+res"]
FUSED_ROUTES = ["lib"] + BLOCK * 2 + (BLOCK + ["conv1x1s2"] + BLOCK) * 3       # module order: conv1, conv2, downsample.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _randomise_norms(net, seed):
    """Running statistics and affine parameters off the identity: identity statistics would hide a wrong fold."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.empty_like(m.weight).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty_like(m.bias).normal_(0, 0.1, generator=g))
                m.running_mean.copy_(torch.empty_like(m.running_mean).normal_(0, 0.1, generator=g))
                m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
    return net


def _net(dev, seed=11, out_vector_size=128):
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    return _randomise_norms(ea.ResNet18Network((3, 32, 32), 8, 3, out_vector_size=out_vector_size), seed + 1).to(dev).eval()


def _ref64(net, xs):
    """The plain route in fp64 on the CPU."""
    net64 = copy.deepcopy(net).double().cpu().eval()
    with torch.no_grad():
        return [net64.resnet18(x.double().cpu()) for x in xs]


def _pooled(outs, refs):
    return sum(float((o.double().cpu() - r).pow(2).sum()) for o, r in zip(outs, refs)) ** 0.5


def _three_ways(net, xs, monkeypatch):
    """(fp64 reference, plain fp32 on the device, fused) outputs for the inputs xs, with the routes each run reported."""
    refs = _ref64(net, xs)
    with torch.no_grad():
        monkeypatch.setenv("EQA_RESNET_KERNEL", "0")
        plain = [net(x) for x in xs]
        routes_plain = list(net.last_routes)
        monkeypatch.delenv("EQA_RESNET_KERNEL")
        fused = [net(x) for x in xs]
        routes_fused = list(net.last_routes)
    return refs, plain, fused, routes_plain, routes_fused


def _inputs(dev, seed=5):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(2, 3, 32, 32, device=dev, generator=g), torch.randn(3, 3, 40, 56, device=dev, generator=g)]


def test_fused_route_is_as_close_to_fp64_as_the_plain_route(dev, monkeypatch):
    """B = 2 at 3 x 32 x 32 and B = 3 at 3 x 40 x 56 (stages 10 x 14, 5 x 7, 3 x 4, 2 x 2): the fused route's distance to the plain route in
    fp64 on the CPU, pooled 2-norm over the two cases, is at most 4 x the plain fp32 route's own on the device (the project's budget
    rule).  Measured at |out|_2 = 26.4: plain 1.24e-5 ... 1.33e-5, fused 1.97e-5."""
    net = _net(dev)
    xs = _inputs(dev)
    refs, plain, fused, routes_plain, routes_fused = _three_ways(net, xs, monkeypatch)
    assert routes_plain == ["plain"] * 20 and routes_fused == FUSED_ROUTES, routes_fused
    assert fused[0].shape == (2, 128) and fused[1].shape == (3, 128) and all(bool(torch.isfinite(f).all()) for f in fused)
    d_plain, d_fused = _pooled(plain, refs), _pooled(fused, refs)
    scale = sum(float(r.pow(2).sum()) for r in refs) ** 0.5
    print(f"ResNet18Network: |out|_2 = {scale:.3e}; to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}")
    assert d_fused <= 4 * d_plain, (d_fused, d_plain)


def test_layers_the_gate_hands_to_the_library_stay_inside_the_budget(dev, monkeypatch):
    """B = 8 at 3 x 128 x 128: stage 2 has 8 x 16 x 16 = 2048 pixels, so its three stride-1 3 x 3 layers (128 channels) take the library's
    convolution ("lib") under the gate on shapes while everything else stays on the kernel; the same budget holds."""
    net = _net(dev)
    xs = [torch.randn(8, 3, 128, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(9))]
    refs, plain, fused, routes_plain, routes_fused = _three_ways(net, xs, monkeypatch)
    want = list(FUSED_ROUTES)
    for slot in (6, 8, 9):                                       # layer2.0.conv2, layer2.1.conv1, layer2.1.conv2
        want[slot] = "lib"
    assert routes_fused == want, routes_fused
    d_plain, d_fused = _pooled(plain, refs), _pooled(fused, refs)
    print(f"gated: to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}")
    assert d_fused <= 4 * d_plain, (d_fused, d_plain)


def test_what_the_fused_rule_does_not_take_is_the_plain_route_bit_for_bit(dev, monkeypatch):
    """EQA_RESNET_KERNEL=0, gradients enabled, a batch-norm or the module in train(), a forward hook on a bypassed submodule: the plain
    route, whose output is `net.resnet18(x)` bit for bit.  Two separate calls of the library's own ops at the same operands were seen
    to differ in the last bits on the device, so the comparison is with what `net.resnet18` returned inside the very call (its
    forward is wrapped, which is no hook: the entry rule does not see it), and a second call of the module must agree to rounding."""
    net = _net(dev)
    x = _inputs(dev)[0]
    seen = []
    inner = net.resnet18.forward

    def recording(inp):
        seen.append((inp, inner(inp)))
        return seen[-1][1]

    monkeypatch.setattr(net.resnet18, "forward", recording)

    def plain_and_equal():
        seen.clear()
        out = net(x)
        assert net.last_routes == ["plain"] * 20 and len(seen) == 1 and seen[0][0] is x
        assert torch.equal(out, seen[0][1])
        return out

    with torch.no_grad():
        net(x)
        assert net.last_routes == FUSED_ROUTES and not seen
        monkeypatch.setenv("EQA_RESNET_KERNEL", "0")
        out = plain_and_equal()
        assert torch.allclose(out, inner(x), rtol=0, atol=1e-5 * out.abs().max().item())
        monkeypatch.delenv("EQA_RESNET_KERNEL")
    assert plain_and_equal().requires_grad                                  # gradients enabled
    with torch.no_grad():
        net.resnet18.layer3[1].bn2.train()                                  # one batch-norm in training mode
        plain_and_equal()
        net.resnet18.layer3[1].bn2.eval()
        handle = net.resnet18.layer2[0].conv2.register_forward_hook(lambda m, i, o: None)
        plain_and_equal()                                                   # a hook on a submodule the fused route would bypass
        handle.remove()
        seen.clear()
        net(x)
        assert net.last_routes == FUSED_ROUTES and not seen
        net.train()
        mean_before = net.resnet18.bn1.running_mean.clone()
        plain_and_equal()
        assert not torch.equal(net.resnet18.bn1.running_mean, mean_before)    # (batch statistics: the modules ran as constructed)


def test_folded_operands_follow_every_change_of_their_sources(dev, monkeypatch):
    """After an in-place change of a convolution weight and of a running_var, an assignment bn.weight = nn.Parameter(...) and a
    load_state_dict, the fused output is within the budget of the new plain route; the fused output from before the change is not."""
    net = _net(dev)
    xs = _inputs(dev)[:1]

    def change_inplace(n):
        with torch.no_grad():
            n.resnet18.layer2[0].conv1.weight.mul_(1.5)
            n.resnet18.layer3[0].downsample[1].running_var.mul_(3.0)

    def change_assign(n):
        bn = n.resnet18.layer1[1].bn2
        bn.weight = torch.nn.Parameter(torch.full_like(bn.weight, 0.25))

    def change_load(n):
        n.load_state_dict(_net(dev, seed=23).state_dict())

    with torch.no_grad():
        before = [net(x) for x in xs]
    assert net.last_routes == FUSED_ROUTES
    for change in (change_inplace, change_assign, change_load):
        change(net)
        refs, plain, fused, _, routes_fused = _three_ways(net, xs, monkeypatch)
        assert routes_fused == FUSED_ROUTES
        d_plain, d_fused, d_stale = _pooled(plain, refs), _pooled(fused, refs), _pooled(before, refs)
        print(f"{change.__name__}: to fp64: plain {d_plain:.3e}, fused {d_fused:.3e}, the output from before the change {d_stale:.3e}")
        assert d_fused <= 4 * d_plain, (change.__name__, d_fused, d_plain)
        assert d_stale > 4 * d_plain, (change.__name__, d_stale, d_plain)
        before = fused


def test_a_training_step_runs_plain_and_the_next_eval_forward_is_fused_on_the_new_weights(dev, monkeypatch):
    net = _net(dev).train()
    x = torch.randn(4, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    out = net(x)
    assert net.last_routes == ["plain"] * 20 and out.requires_grad
    (out * torch.randn_like(out)).sum().backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    with torch.no_grad():
        net.eval()
        stale = [net(x)]                                       # (fills the cache with the weights from before the step)
        assert net.last_routes == FUSED_ROUTES
    opt.step()
    refs, plain, fused, _, routes_fused = _three_ways(net, [x], monkeypatch)
    assert routes_fused == FUSED_ROUTES
    d_plain, d_fused = _pooled(plain, refs), _pooled(fused, refs)
    assert d_fused <= 4 * d_plain and _pooled(stale, refs) > 4 * d_plain, (d_fused, d_plain)


def test_optimized_canonicalizer_end_to_end(dev, monkeypatch):
    """OptimizedGroupEquivariantImageCanonicalization, D4 (roto-reflection, 4 rotations), resize_shape = 32, input (2, 3, 64, 64): fused
    against forced-plain.  With V the (G B, 128) embeddings, the budget |V_fused - V_plain|_F <= 5 |V_plain - V_fp64|_F =: D enters an
    activation cos(ref, v) by at most D / |v| to first order (the cosine's gradient in v has norm <= 1 / |v|); the bound below is twice
    that plus the fp32 rounding of the cosine itself (a 128-term dot product and two norms of values <= 1: 2^-16 covers it).  Where the
    two runs pick the same element the images are bit-equal; above a top-2 margin of 1e-4 they must pick the same.  The captured
    hipGraph of the step replays the eager fused step bit for bit."""
    import equiadapt_amd as ea
    from equiadapt_amd.graphs import GraphedCanonicalizer

    net = _net(dev, seed=31)
    hp = types.SimpleNamespace(beta=1.0, input_crop_ratio=1.0, resize_shape=32, group_type="roto-reflection", num_rotations=4,
                               artifact_err_wt=0.0, learn_ref_vec=False)
    torch.manual_seed(31)
    can = ea.OptimizedGroupEquivariantImageCanonicalization(net, hp, (3, 64, 64)).to(dev).eval()
    # seed 7: the two images' top-2 margins on the plain route are 2.4e-3 and 1.2e-2 (measured on the MI355X), both above 1e-4
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(7)).to(dev)

    def run():
        with torch.no_grad():
            y = can(x)
        info = can.canonicalization_info_dict
        return y, info["group_activations"].clone(), info["group_index"].clone(), info["vector_out"].clone(), list(net.last_routes)

    monkeypatch.setenv("EQA_RESNET_KERNEL", "0")
    y_p, a_p, g_p, v_p, r_p = run()
    monkeypatch.delenv("EQA_RESNET_KERNEL")
    y_f, a_f, g_f, v_f, r_f = run()
    assert r_p == ["plain"] * 20 and r_f == FUSED_ROUTES
    assert y_f.shape == (2, 3, 64, 64) and a_f.shape == (2, 8) and v_f.shape == (16, 128)
    with torch.no_grad():
        views = can.group_augment(can.transformations_before_canonicalization_network_forward(x))
    v64 = _ref64(net, [views])[0]
    D = 5 * float((v_p.double().cpu() - v64).norm())
    tol = 2 * D / float(v64.norm(dim=1).min()) + 2.0 ** -16
    top2 = a_p.topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]).cpu()
    print(f"activations: |fused - plain| <= {(a_f - a_p).abs().max().item():.3e} (bound {tol:.3e}); top-2 margins on the plain route {margin.tolist()}")
    assert (a_f - a_p).abs().max().item() <= tol
    assert bool((margin > 1e-4).all()), margin
    assert torch.equal(g_f.cpu()[margin > 1e-4], g_p.cpu()[margin > 1e-4])
    same = (g_f == g_p).cpu()
    assert torch.equal(y_f[same], y_p[same])
    step = GraphedCanonicalizer(can, x.shape)
    got = step(x)
    torch.cuda.synchronize()
    assert net.last_routes == FUSED_ROUTES
    assert torch.equal(got[0], y_f) and torch.equal(got[1], g_f)
