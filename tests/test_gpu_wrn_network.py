"""eqa_gconv1x1_nhwc (csrc/gconv1x1.hip) against an fp64 product on the device, and ESCNNWRNEquivariantNetwork's fused route against
its plain route in fp64 (the route tests/test_wrn_network.py holds to a dense evaluation on the CPU): outputs, equivariance, training
through the plain route, and a canonicalizer end to end."""
import copy
import itertools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3      # EQA_ERR_UNSUPPORTED (include/eqa_hip.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


# -- the kernel -------------------------------------------------------------------------------------------------------------------
# pixel counts off the 64-row wave tile (one row, one short of a tile, two tiles and a part, 65 tiles: more than one wave per
# column tile) x channel pairs with one and two 32-column subtiles per wave, Cin != Cout both ways; the widest pair at P = 63
KERNEL_CASES = [(P, ci, co) for P in (1, 63, 162, 4097) for ci, co in ((32, 32), (64, 32), (32, 96), (128, 128))] + [(63, 512, 512)]


def _operands(dev, P, Cin, Cout):
    g = torch.Generator(device=dev).manual_seed(1000 * Cin + Cout + P)

    def rn(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    return rn(P, Cin), rn(Cout, Cin) / Cin ** 0.5, rn(Cout), rn(P, Cout), rn(Cout), rn(Cout)


@pytest.mark.parametrize("P,Cin,Cout", KERNEL_CASES)
def test_kernel_stays_inside_the_dot_product_bound(dev, P, Cin, Cout):
    """Every output within (Cin + 6) 2^-24 (|s| (sum |x||w| + |bias| + |res|) + |t|) of the fp64 evaluation of the same fp32 operands:
    the bound of a Cin-term dot product summed in any order, plus the bias, the residual, the two operations of the affine map and
    their roundings (ReLU is 1-Lipschitz).  All four combinations of residual and affine map, ReLU on and off."""
    from equiadapt_amd import ops

    assert ops.gconv1x1_supported(P, Cin, Cout)
    x, W, bias, res, s, t = _operands(dev, P, Cin, Cout)
    wpk = ops.pack_gconv1x1_weights(W)
    assert wpk.shape == (Cin // 16, Cout // 32, 2, 2, 32, 4)
    dot = torch.einsum("pc,oc->po", x.double(), W.double())
    mag = torch.einsum("pc,oc->po", x.double().abs(), W.double().abs())
    worst = 0.0
    for has_res, has_aff, relu in itertools.product((False, True), repeat=3):
        y = ops.gconv1x1_nhwc(x, wpk, bias, res if has_res else None, s if has_aff else None, t if has_aff else None, relu)
        assert y.shape == (P, Cout) and y.dtype == torch.float32
        z = dot + bias.double() + (res.double() if has_res else 0.0)
        inner = mag + bias.double().abs() + (res.double().abs() if has_res else 0.0)
        if has_aff:
            want, bound = s.double() * z + t.double(), s.double().abs() * inner + t.double().abs()
        else:
            want, bound = z, inner
        if relu:
            want = want.clamp_min(0.0)
        bound = (Cin + 6) * 2.0 ** -24 * bound
        err = (y.double() - want).abs()
        worst = max(worst, (err / bound).max().item())
        assert bool((err <= bound).all()), (P, Cin, Cout, has_res, has_aff, relu, (err / bound).max().item())
        if relu:
            assert y.min().item() >= 0.0
    print(f"gconv1x1 P={P} {Cin}->{Cout}: largest error / bound over the eight forms = {worst:.3f}")


@pytest.mark.parametrize("P,Cin,Cout", [(1, 32, 32), (63, 64, 32), (162, 32, 96), (4097, 128, 128)])
def test_rows_past_the_pixel_count_are_never_stored(dev, P, Cin, Cout):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    x, W, bias, res, s, t = _operands(dev, P, Cin, Cout)
    wpk = ops.pack_gconv1x1_weights(W)
    want = ops.gconv1x1_nhwc(x, wpk, bias, res, s, t, True)
    big_x = torch.cat([x, torch.full((70, Cin), 3.0, device=dev)])          # (what lies behind the last row must not be read into it)
    big_r = torch.cat([res, torch.full((70, Cout), 5.0, device=dev)])
    y = torch.full((P + 70, Cout), 7.0, device=dev)
    st = lib.eqa_gconv1x1_nhwc(big_x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), big_r.data_ptr(), s.data_ptr(), t.data_ptr(), 1, y.data_ptr(),
                               P, Cin, Cout, None)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:P], want)
    assert bool((y[P:] == 7.0).all()), "rows beyond the pixel count must not be written"


def test_channels_last_map_and_its_matrix_give_the_same_bits(dev):
    from equiadapt_amd import ops

    x, W, bias, res, s, t = _operands(dev, 162, 64, 96)
    wpk = ops.pack_gconv1x1_weights(W[:, :, None, None])
    xm = x.view(2, 9, 9, 64).permute(0, 3, 1, 2)
    rm = res.view(2, 9, 9, 96).permute(0, 3, 1, 2)
    y = ops.gconv1x1_nhwc(xm, wpk, bias, rm, s, t, True)
    assert y.shape == (2, 96, 9, 9) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(162, 96), ops.gconv1x1_nhwc(x, wpk, bias, res, s, t, True))
    with pytest.raises(RuntimeError):
        ops.gconv1x1_nhwc(xm.contiguous(), wpk, bias)                       # not channels-last
    with pytest.raises(ValueError):
        ops.gconv1x1_nhwc(x, wpk, bias, None, s, None)


def test_what_the_query_refuses_is_never_launched(dev):
    """Channel counts off the multiples of 32 or above 512, and a map past the 32-bit buffer range: the query says no (and the entry
    point, given the same sizes and no memory at all, answers EQA_ERR_UNSUPPORTED before it looks at a pointer)."""
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    refused = [(100, 48, 64), (100, 64, 544), (2 ** 21, 64, 512), (2 ** 21, 512, 64), (100, 16, 32), (100, 32, 0)]
    for P, ci, co in refused:
        assert not ops.gconv1x1_supported(P, ci, co), (P, ci, co)
    for P, ci, co in refused[:4]:
        assert lib.eqa_gconv1x1_nhwc(None, None, None, None, None, None, 0, None, P, ci, co, None) == UNSUPPORTED
    assert ops.gconv1x1_supported(2 ** 21 - 1, 64, 512) and ops.gconv1x1_supported(0, 32, 32) and ops.gconv1x1_supported(7, 512, 512)


# -- the network ------------------------------------------------------------------------------------------------------------------
def _net(dev, group, out_channels, in_shape=(3, 33, 33), k=3, layers=6, seed=11):
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    net = ea.ESCNNWRNEquivariantNetwork(in_shape, out_channels, k, group, layers, 4)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "expanded_weights"):
                m.bias.normal_(0, 0.1)
            if isinstance(m, torch.nn.BatchNorm3d):               # running statistics (and the affine map) randomised
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return net.to(dev).eval()


def _turned(out, q, group):
    """What a network's (B, |G|) output becomes when its input is turned by q quarter turns: the rotations shift by q, the
    reflected half by -q."""
    if group == "rotation":
        return out.roll(q, dims=1)
    return torch.cat([out[:, :4].roll(q, dims=1), out[:, 4:].roll(-q, dims=1)], dim=1)


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


_RUNS = {}


def _runs(dev, group, out_channels, in_shape=(3, 33, 33), k=3):
    """One evaluation per configuration, shared by the tests below: the input and its three turns through the plain route in fp64 and
    in fp32 (EQA_WRN_KERNEL=0) and through the fused route."""
    import os

    key = (group, out_channels, in_shape, k)
    if key in _RUNS:
        return _RUNS[key]
    net = _net(dev, group, out_channels, in_shape, k)
    net64 = copy.deepcopy(net).double()
    x = torch.randn(2, *in_shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    xs = [torch.rot90(x, q, (2, 3)).contiguous() for q in range(4)]
    old = os.environ.get("EQA_WRN_KERNEL")
    try:
        with torch.no_grad():
            ref = [net64(v.double()) for v in xs]
            routes64 = list(net64.last_routes)
            os.environ["EQA_WRN_KERNEL"] = "0"
            plain = [net(v).double() for v in xs]
            routes_plain = list(net.last_routes)
            os.environ["EQA_WRN_KERNEL"] = "1"
            fused = [net(v).double() for v in xs]
            routes_fused = list(net.last_routes)
    finally:
        if old is None:
            os.environ.pop("EQA_WRN_KERNEL", None)
        else:
            os.environ["EQA_WRN_KERNEL"] = old
    _RUNS[key] = types.SimpleNamespace(net=net, ref=ref, plain=plain, fused=fused, routes64=routes64, routes_plain=routes_plain,
                                       routes_fused=routes_fused, group=group)
    return _RUNS[key]


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_fused_route_is_as_close_to_fp64_as_the_plain_route(dev, group):
    """out_channels = 32: 32 to 256 channels, every bottleneck 1 x 1 on the kernel.  The fused route's distance to the plain route in
    fp64 is at most 4 x the plain fp32 route's own (its k x k layers sum in another order).  Measured at |out| <= 1.2e-2 (DESIGN.md
    section 1, "ESCNNWRNEquivariantNetwork"): C4 plain 2.3e-9, fused 1.0e-9 ... 1.2e-9; D4 plain 5.8e-9, fused 2.2e-9 ... 3.1e-9."""
    r = _runs(dev, group, 32)
    E = 4 if group == "rotation" else 8
    assert r.ref[0].shape == (2, E) and bool(torch.isfinite(r.ref[0]).all())
    assert set(r.routes64) == {"conv2d"} and set(r.routes_plain) == {"conv2d"} and len(r.routes_fused) == len(r.routes_plain) == 17
    for first, second in _one_by_ones(r.net):
        assert (r.routes_fused[first], r.routes_fused[second]) == ("gconv1x1", "gconv1x1+junction"), r.routes_fused
    assert r.routes_fused[-1] == "window_sums"
    d_plain = (r.plain[0] - r.ref[0]).abs().max().item()
    d_fused = (r.fused[0] - r.ref[0]).abs().max().item()
    print(f"{group}: |out| <= {r.ref[0].abs().max().item():.3e}; to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}; routes {r.routes_fused}")
    assert d_fused <= 4 * d_plain, (d_fused, d_plain)


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_layers_below_the_gate_take_the_plain_ops_and_the_rest_stays_fused(dev, group):
    """out_channels = 8: 8 to 32 (C4) / 16 to 64 (D4) channels -- the first bottleneck's 1 x 1 layers are too narrow for the kernel,
    the last one's are not.  Same tolerance.  Measured: C4 plain 2.3e-9, fused 9.8e-10; D4 plain 5.7e-9, fused 2.6e-9 ... 4.7e-9."""
    r = _runs(dev, group, 8)
    ones = [r.routes_fused[i] for pair in _one_by_ones(r.net) for i in pair]
    assert "lib" in ones and "gconv1x1" in ones and "gconv1x1+junction" in ones, r.routes_fused
    d_plain = (r.plain[0] - r.ref[0]).abs().max().item()
    d_fused = (r.fused[0] - r.ref[0]).abs().max().item()
    print(f"{group} (8): to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}; routes {r.routes_fused}")
    assert d_fused <= 4 * d_plain, (d_fused, d_plain)


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_quarter_turn_banks_are_exact_permutations_of_the_filter_taps(dev, group):
    """The network's layers expand their filters by exact quarter turns and flips: the package's bilinear fp32 action matrices (up to
    4e-7 off at k = 3) are within 1e-5 of a permutation matrix, to which they are rounded.  Every element's filter of the stem is a
    rot90 / flip image of the stored filter, bit for bit, the images of one filter differ, and a group convolution's bank holds
    nothing but stored taps."""
    from equiadapt_amd.images.canonicalization_networks import custom_group_equivariant_layers as cgl

    refl = group == "roto-reflection"
    A = cgl.filter_action_matrices(3, 4, refl, dev)
    off = (A - A.round()).abs().max().item()
    print(f"{group}: the package's action matrices are {off:.3e} off their rounding")
    assert off <= 1e-5
    R = A.round()
    assert bool(((R == 0) | (R == 1)).all()) and bool((R.sum(-1) == 1).all()) and bool((R.sum(-2) == 1).all())
    net = _net(dev, group, 32)
    stem = net.eqv_network[0]
    E, O, I, k = stem.num_group_elements, stem.out_channels, stem.in_channels, stem.kernel_size
    with torch.no_grad():
        w = stem.weights
        bank = stem.expanded_weights().view(O, E, I, k, k)
        images = [torch.rot90(v, r, (2, 3)) for v in ((w, w.flip(3)) if refl else (w,)) for r in range(4)]
        hit = [[j for j, im in enumerate(images) if torch.equal(bank[:, e], im)] for e in range(E)]
        assert all(len(h) == 1 for h in hit) and sorted(h[0] for h in hit) == list(range(E)), hit
        conv = net.eqv_network[-1]
        assert bool(torch.isin(conv.expanded_weights(), conv.weights).all())


def _equivariance_error(outs, group):
    return max((outs[q] - _turned(outs[0], q, group)).abs().max().item() for q in (1, 2, 3))


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_quarter_turns_permute_the_plain_fp64_output(dev, group):
    """Plain fp64 route: net(rot90(x, q)) is the permuted net(x) to 1e-9.  (With the package's bilinear fp32 action matrices, up to
    3.6e-7 off a permutation at k = 3, the same networks measured 7.5e-10 (C4) and 4.5e-9 (D4) at |out| <= 1.2e-2; the network's layers
    round them to the permutations, wrn_networks._ExactQuarterTurns, and measure 5e-18 and 7e-18.)"""
    r = _runs(dev, group, 32)
    e64 = _equivariance_error(r.ref, group)
    print(f"{group}: equivariance error of the plain fp64 route {e64:.3e} at |out| <= {r.ref[0].abs().max().item():.3e}")
    assert (r.ref[1] - r.ref[0]).abs().max().item() > 1e-6, "the turn must be visible in the output"
    assert e64 <= 1e-9


@pytest.mark.parametrize("group", ["rotation", "roto-reflection"])
def test_fused_route_is_as_equivariant_as_the_plain_route(dev, group):
    """The fused route's equivariance error is at most 4 x the plain fp32 route's own.  Measured: C4 plain 1.9e-9, fused 1.9e-9;
    D4 plain 4.7e-9 ... 5.6e-9, fused 2.8e-9 ... 3.7e-9."""
    r = _runs(dev, group, 32)
    e_plain, e_fused = _equivariance_error(r.plain, group), _equivariance_error(r.fused, group)
    print(f"{group}: equivariance error: plain fp32 {e_plain:.3e}, fused {e_fused:.3e}")
    assert e_fused <= 4 * e_plain, (e_fused, e_plain)


def test_k5_layers_on_the_winograd_or_fft_convolution(dev):
    """kernel_size = 5 at 40 x 40: the bottlenecks' padded 5 x 5 layers (32, 64, 128 channels) are shapes the Winograd / FFT
    convolutions take.  Those kernels are held to 2e-5 of their output's scale per layer (test_gpu_parity.py, the Winograd test), so
    the fused route is allowed the plain route's distance plus that per such layer, relative to the output's scale, times the same 4.
    Measured at |out| <= 1.3e-2: plain 3.8e-9, fused 4.9e-9 (the seven 5 x 5 layers on "wino", the two 9 x 9 shortcuts on "lib")."""
    r = _runs(dev, "rotation", 32, (3, 40, 40), 5)
    taken = [v for v in r.routes_fused if v in ("wino", "fft5")]
    assert taken, r.routes_fused
    for first, second in _one_by_ones(r.net):
        assert (r.routes_fused[first], r.routes_fused[second]) == ("gconv1x1", "gconv1x1+junction"), r.routes_fused
    d_plain = (r.plain[0] - r.ref[0]).abs().max().item()
    d_fused = (r.fused[0] - r.ref[0]).abs().max().item()
    scale = r.ref[0].abs().max().item()
    print(f"k = 5: |out| <= {scale:.3e}; to fp64: plain fp32 {d_plain:.3e}, fused {d_fused:.3e}; routes {r.routes_fused}")
    assert d_fused <= 4 * (d_plain + len(taken) * 2e-5 * scale), (d_fused, d_plain)


def test_training_takes_the_plain_route(dev):
    """One train() forward and backward at (2, 3, 21, 21), num_layers = 3: plain route, a finite gradient for every parameter, running
    statistics updated with momentum 0.9 (new = 0.1 old + 0.9 batch)."""
    import torch.nn.functional as F

    net = _net(dev, "rotation", 8, (3, 21, 21), 3, 3).train()
    norms = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    old = [m.running_mean.clone() for m in norms]
    x = torch.randn(2, 3, 21, 21, device=dev)
    out = net(x)
    assert out.shape == (2, 4) and out.requires_grad and set(net.last_routes) == {"conv2d"} and len(net.last_routes) == 8
    (out * torch.randn_like(out)).sum().backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert sum(float(p.grad.abs().sum()) > 0 for p in net.parameters()) > len(list(net.parameters())) // 2
    for m, o in zip(norms, old):
        assert int(m.num_batches_tracked) == 1 and (m.running_mean - o).abs().max().item() > 1e-4
    with torch.no_grad():
        stem = net.eqv_network[0]
        y = F.conv2d(x, stem.expanded_weights()).view(2, stem.out_channels, 4, 19, 19) + stem.bias[None, :, None, None, None]
        want = 0.1 * old[0] + 0.9 * y.mean(dim=(0, 2, 3, 4))
    assert (norms[0].running_mean - want).abs().max().item() <= 1e-5
    net.eval()
    with torch.no_grad():
        net(x)
    assert "conv2d" not in net.last_routes                        # back in eval under no_grad: the fused route


def test_canonicalizer_end_to_end(dev):
    """GroupEquivariantImageCanonicalization on the network: canonicalize and invert a (2, 3, 40, 40) batch (crop 0.8 -> 32, resize to
    33), against the CPU oracle for the element the network picked."""
    import equiadapt_amd as ea
    from oracle import image_ops as io

    net = _net(dev, "rotation", 32)
    hp = types.SimpleNamespace(beta=1.0, input_crop_ratio=0.8, resize_shape=33)
    can = ea.GroupEquivariantImageCanonicalization(net, hp, (3, 40, 40)).to(dev).eval()
    torch.manual_seed(9)
    x, f = torch.randn(2, 3, 40, 40), torch.randn(2, 4, 40, 40)
    with torch.no_grad():
        y = can(x.to(dev))
        inv = can.invert_canonicalization(f.to(dev), induced_rep_type="regular")
    assert "gconv1x1+junction" in net.last_routes
    acts = can.canonicalization_info_dict["group_activations"]
    gidx = can.canonicalization_info_dict["group_index"].cpu().long()
    assert acts.shape == (2, 4) and torch.equal(gidx, acts.argmax(dim=1).cpu())
    ang = io.group_angles(4)[gidx]
    e1 = (y.cpu() - io.canonicalize_images(x, ang, None, (3, 40, 40))).abs().max().item()
    e2 = (inv.cpu() - io.invert_action(f, ang, None, 4, 4, "regular")).abs().max().item()
    assert y.shape == x.shape and inv.shape == f.shape and e1 < 1e-3 and e2 < 1e-3, (e1, e2)
