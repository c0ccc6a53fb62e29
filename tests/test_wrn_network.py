"""CPU: the construction of ESCNNWRNEquivariantNetwork (names, layer plan against a table, argument checks, checkpoint refusal) and,
at kernel_size = 1 -- the only size whose filter banks need no device --, its wiring in fp64 against a per-pixel dense evaluation
written here.  The device routes are held to this plain route in tests/test_gpu_wrn_network.py."""
import pytest
import torch

import equiadapt_amd as ea
from equiadapt_amd.images.canonicalization_networks import wrn_networks as wn

# (in_shape, out_channels, kernel_size, group_type, num_layers, num_rotations) and what the reference's constructor
# (escnn_networks.py:430-483) builds from it: |G|, then per module of eqv_network that holds convolutions
#   (kind, (in, middle, out) fields, kernel sizes, paddings) -- a bottleneck's 1 x 1, k x k, 1 x 1; a basic block's two k x k and its shortcut
RECIPE = ((3, 128, 128), 64, 5, "rotation", 12, 4)
RECIPE_PLAN = (4, [("lift", (3, 16), (5,), (0,))]
               + [("bottleneck", (16, 16, 16), (1, 5, 1), (0, 2, 0))] * 3 + [("basic", (16, 32, 32), (5, 5, 9), (0, 0, 0))]
               + [("bottleneck", (32, 32, 32), (1, 5, 1), (0, 2, 0))] * 3 + [("basic", (32, 64, 64), (5, 5, 9), (0, 0, 0))]
               + [("bottleneck", (64, 64, 64), (1, 5, 1), (0, 2, 0))] * 3 + [("conv", (64, 128), (5,), (0,))])
SMALL = ((3, 33, 33), 32, 3, "roto-reflection", 6, 4)
SMALL_PLAN = (8, [("lift", (3, 8), (3,), (0,)),
                  ("bottleneck", (8, 8, 8), (1, 3, 1), (0, 1, 0)), ("basic", (8, 16, 16), (3, 3, 5), (0, 0, 0)),
                  ("bottleneck", (16, 16, 16), (1, 3, 1), (0, 1, 0)), ("basic", (16, 32, 32), (3, 3, 5), (0, 0, 0)),
                  ("bottleneck", (32, 32, 32), (1, 3, 1), (0, 1, 0)), ("conv", (32, 64), (3,), (0,))])


def _convs(block):
    return [m for m in block.modules() if hasattr(m, "expanded_weights")]


def _plan(net):
    """The table above, read off the modules."""
    rows, mods = [], list(net.eqv_network)
    for i, m in enumerate(mods):
        if isinstance(m, (ea.ESCNNWideBottleneck, ea.ESCNNWideBasic)):
            cs = _convs(m)
            kind = "bottleneck" if isinstance(m, ea.ESCNNWideBottleneck) else "basic"
            assert (m.in_fields, m.middle_fields, m.out_fields) == (cs[0].in_channels, cs[0].out_channels, cs[1].out_channels)
            assert cs[2].in_channels == (m.out_fields if kind == "bottleneck" else m.in_fields)
            assert cs[2].out_channels == (m.in_fields if kind == "bottleneck" else m.out_fields)
            assert not any(c.lifting for c in cs) and all(c.bias is not None and c.stride == 1 for c in cs)
            norms = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm3d)]
            assert [b.num_features for b in norms] == ([m.middle_fields, m.out_fields] if kind == "bottleneck" else [m.middle_fields])
            rows.append((kind, (m.in_fields, m.middle_fields, m.out_fields), tuple(c.kernel_size for c in cs), tuple(c.padding for c in cs)))
        elif hasattr(m, "expanded_weights"):
            assert m.lifting == (i == 0) and m.bias is not None and m.stride == 1
            rows.append(("lift" if m.lifting else "conv", (m.in_channels, m.out_channels), (m.kernel_size,), (m.padding,)))
        if hasattr(m, "expanded_weights") or isinstance(m, (ea.ESCNNWideBottleneck, ea.ESCNNWideBasic)):
            if i + 1 < len(mods):                 # InnerBatchNorm(momentum = 0.9, affine) over the block's output fields, then ReLU
                bn = mods[i + 1]
                assert isinstance(bn, torch.nn.BatchNorm3d) and bn.momentum == 0.9 and bn.affine and isinstance(mods[i + 2], torch.nn.ReLU)
                assert bn.num_features == (rows[-1][1][0] if rows[-1][0] == "bottleneck" else rows[-1][1][-1])
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            assert m.momentum == 0.9 and m.affine
        assert not isinstance(m, torch.nn.Dropout)
    return net.num_group_elements, rows


def test_names_resolve_and_are_exported():
    for name in ("ESCNNWRNEquivariantNetwork", "ESCNNWideBottleneck", "ESCNNWideBasic"):
        assert getattr(ea, name) is getattr(wn, name) is getattr(ea.escnn_networks, name)
        assert name in ea.__all__
    from equiadapt_amd.images import canonicalization_networks as cn

    assert cn.ESCNNWRNEquivariantNetwork is ea.ESCNNWRNEquivariantNetwork


@pytest.mark.parametrize("cfg,plan", [(RECIPE, RECIPE_PLAN), (SMALL, SMALL_PLAN)], ids=["recipe", "small_d4"])
def test_layer_plan_matches_the_reference_constructor(cfg, plan):
    in_shape, oc, k, group, layers, nrot = cfg
    net = ea.ESCNNWRNEquivariantNetwork(in_shape, oc, k, group, layers, nrot)
    assert _plan(net) == plan
    assert (net.out_channels, net.kernel_size, net.group_type, net.num_rotations, net.num_group_elements) == (2 * oc, k, group, nrot, plan[0])
    assert len(net.eqv_network) == 3 * layers + 1 and net.last_routes == []


def test_defaults_are_the_reference_s():
    import inspect

    sig = inspect.signature(ea.ESCNNWRNEquivariantNetwork.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[2:]] == [("out_channels", 64), ("kernel_size", 9), ("group_type", "rotation"),
                                                                  ("num_layers", 12), ("num_rotations", 4)]
    for cls in (ea.ESCNNWideBottleneck, ea.ESCNNWideBasic):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == ["in_fields", "middle_fields", "out_fields", "kernel_size", "group_type",
                                                                        "num_rotations"]


@pytest.mark.parametrize("layers", [4, 2])
def test_num_layers_the_reference_would_index_past_raises(layers):
    with pytest.raises(ValueError, match="multiple of 3"):
        ea.ESCNNWRNEquivariantNetwork((3, 33, 33), 8, 3, "rotation", layers, 4)


def test_three_layers_have_no_bottleneck():
    net = ea.ESCNNWRNEquivariantNetwork((3, 21, 21), 8, 3, "rotation", 3, 4)
    assert [r[0] for r in _plan(net)[1]] == ["lift", "basic", "basic", "conv"]


def test_bad_group_type_raises_with_the_reference_message():
    with pytest.raises(ValueError, match="group_type must be rotation or roto-reflection for now."):
        ea.ESCNNWRNEquivariantNetwork((3, 33, 33), 8, 3, "dihedral", 6, 4)
    with pytest.raises(ValueError, match="group_type must be rotation or roto-reflection for now."):
        ea.ESCNNWideBasic(2, 4, 4, 3, "dihedral", 4)


def test_e2cnn_checkpoint_raises_and_says_why():
    net = ea.ESCNNWRNEquivariantNetwork((3, 9, 9), 8, 1, "rotation", 3, 4)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(sd)                                     # its own state dict loads
    assert "eqv_network.3.conv_network.0.weights" in sd and "eqv_network.3.shortcut.0.bias" in sd
    for key, val in (("eqv_network.3.conv_network.0.weights", torch.zeros(24)),     # e2cnn: one flat coefficient vector per layer
                     ("eqv_network.0.basisexpansion.block_expansion_('irrep_0', 'regular').sampled_basis", torch.zeros(1)),
                     ("eqv_network.9.filter", torch.zeros(1))):
        bad = dict(sd)
        bad[key] = val
        with pytest.raises(RuntimeError, match="steerable-basis parameterisation.*cannot load it by key"):
            net.load_state_dict(bad, strict=False)


# -- wiring at kernel_size = 1, C4, fp64 ------------------------------------------------------------------------------------------
def _wired_net():
    torch.manual_seed(3)
    net = ea.ESCNNWRNEquivariantNetwork((3, 5, 5), 8, 1, "rotation", 6, 4).double()
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "expanded_weights"):
                m.bias.normal_(0, 0.3)
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.3)
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    return net.eval()


def _dense(conv):
    """(matrix (out channels, in channels), bias per out channel) of a 1 x 1 C4 layer, channel = field * 4 + element: the lifting
    layer copies its filter to every element; a group convolution reads input slot m of output element e from stored slot
    (m - e) mod 4 (reference custom_group_equivariant_layers.py:283-293)."""
    w = conv.weights.detach()
    O, I = w.shape[:2]
    if conv.lifting:
        M = torch.zeros(O, 4, I, dtype=w.dtype)
        for e in range(4):
            M[:, e] = w[:, :, 0, 0]
        return M.reshape(O * 4, I), conv.bias.detach().repeat_interleave(4)
    M = torch.zeros(O, 4, I, 4, dtype=w.dtype)
    for e in range(4):
        for m in range(4):
            M[:, e, :, m] = w[:, :, (m - e) % 4, 0, 0]
    return M.reshape(O * 4, I * 4), conv.bias.detach().repeat_interleave(4)


def _dense_forward(net, x):
    """Per pixel, on (pixels, channels) matrices."""
    def lin(conv, v):
        M, b = _dense(conv)
        return v @ M.t() + b

    def bn(norm, v):
        s = (norm.weight / torch.sqrt(norm.running_var + norm.eps)).detach()
        return v * s.repeat_interleave(4) + (norm.bias - norm.running_mean * s).detach().repeat_interleave(4)

    B, C, H, W = x.shape
    mods = list(net.eqv_network)
    v = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
    v = torch.relu(bn(mods[1], lin(mods[0], v)))
    for i in range(3, len(mods) - 1, 3):
        blk, cn = mods[i], list(mods[i].conv_network)
        if isinstance(blk, ea.ESCNNWideBottleneck):
            u = torch.relu(bn(cn[1], lin(cn[0], v)))
            u = torch.relu(bn(cn[4], lin(cn[3], u)))
            z = lin(cn[6], u) + v
        else:
            u = torch.relu(bn(cn[1], lin(cn[0], v)))
            z = lin(cn[3], u) + lin(blk.shortcut[0], v)
        v = torch.relu(bn(mods[i + 1], z))
    v = lin(mods[-1], v)
    return v.reshape(B, H * W, -1, 4).mean(dim=(1, 2))


def test_forward_equals_a_per_pixel_dense_evaluation():
    net = _wired_net()
    x = torch.randn(2, 3, 5, 5, dtype=torch.float64)
    with torch.no_grad():
        got = net(x)
    want = _dense_forward(net, x)
    assert got.shape == (2, 4) and got.dtype == torch.float64
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    assert net.last_routes == ["conv2d"] * 17                   # 1 + 3 * 5 + 1 convolutions, all on the plain route


def test_quarter_turn_rolls_the_output():
    net = _wired_net()
    x = torch.randn(2, 3, 5, 5, dtype=torch.float64)
    with torch.no_grad():
        a, b = net(x), net(torch.rot90(x, 1, (2, 3)))
    assert (b - a.roll(1, dims=1)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("block", ["bottleneck", "basic"])
def test_blocks_commute_with_a_shift_of_the_group_axis(block):
    """A 1 x 1 filter is its own rotation, so at kernel_size = 1 a quarter turn acts on a regular feature map as rot90 of the plane and
    a cyclic shift of the group axis: the blocks must commute with it (a 1 x 1 lifting layer gives every element the same map, so the
    whole network's outputs above cannot tell a shift from none; a random feature map can)."""
    torch.manual_seed(5)
    blk = (ea.ESCNNWideBottleneck(3, 3, 3, 1) if block == "bottleneck" else ea.ESCNNWideBasic(3, 5, 5, 1)).double().eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
        f = torch.randn(2, 3, 4, 5, 5, dtype=torch.float64)

        def act(t):
            return torch.rot90(t, 1, (3, 4)).roll(1, dims=2)

        a, b = act(blk(f)), blk(act(f))
        assert (a - b).abs().max().item() <= 1e-12
        assert (blk(f) - blk(f.roll(1, dims=2))).abs().max().item() > 1e-3     # (the shift is visible)
