"""CPU-only: ResNet18Network's interface, parameter names and plain route, the packed operand layout of the 3 x 3 kernel, and the
argument checks of its entry points that need no device."""
import inspect
import types

import pytest
import torch

INVALID, UNSUPPORTED = -1, -3      # EQA_ERR_INVALID_ARG, EQA_ERR_UNSUPPORTED (include/eqa_hip.h)


def _net(seed=0, **kw):
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    return ea.ResNet18Network((3, 32, 32), 8, 3, **kw)


def _expected_keys():
    """torchvision's resnet18 names under `resnet18.`, from the layer plan: stem, four stages of two basic blocks (a projection
    shortcut in the first block of stages 2-4), and the reference's replacement head fc.0."""
    def bn(p):
        return [f"{p}.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]

    keys = ["conv1.weight"] + bn("bn1")
    for stage in range(1, 5):
        for blk in range(2):
            p = f"layer{stage}.{blk}"
            keys += [f"{p}.conv1.weight"] + bn(f"{p}.bn1") + [f"{p}.conv2.weight"] + bn(f"{p}.bn2")
            if stage > 1 and blk == 0:
                keys += [f"{p}.downsample.0.weight"] + bn(f"{p}.downsample.1")
    keys += ["fc.0.weight", "fc.0.bias"]
    return ["resnet18." + k for k in keys]


def test_constructor_signature_and_attributes():
    import equiadapt_amd as ea
    from equiadapt_amd.images.canonicalization_networks import ResNet18Network, custom_nonequivariant_networks

    assert ea.ResNet18Network is ResNet18Network is custom_nonequivariant_networks.ResNet18Network and "ResNet18Network" in ea.__all__
    params = list(inspect.signature(ResNet18Network.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [("in_shape", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty),
                                                     ("kernel_size", inspect.Parameter.empty), ("num_layers", 2), ("out_vector_size", 128)]
    assert _net().out_vector_size == 128 and _net(out_vector_size=16).out_vector_size == 16
    assert _net(out_vector_size=16).resnet18.fc[0].weight.shape == (16, 512)


def test_state_dict_has_torchvisions_names_and_loads_strictly():
    net = _net()
    sd = net.state_dict()
    assert len(sd) == 122 and list(sd) == _expected_keys()
    assert list(sd)[-2:] == ["resnet18.fc.0.weight", "resnet18.fc.0.bias"]
    assert sum(p.numel() for p in net.parameters()) == 11_242_176
    other = _net(seed=1)
    assert not torch.equal(other.resnet18.conv1.weight, net.resnet18.conv1.weight)
    other.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    for (k, a), b in zip(other.state_dict().items(), sd.values()):
        assert torch.equal(a, b), k


def test_load_torchvision_state_dict_loads_the_backbone_and_leaves_the_head():
    net, donor = _net(), _net(seed=1)
    with torch.no_grad():
        donor.resnet18.bn1.running_mean.normal_()
    tv = {k: v.clone() for k, v in donor.resnet18.state_dict().items() if not k.startswith("fc.")}
    tv["fc.weight"], tv["fc.bias"] = torch.randn(1000, 512), torch.randn(1000)
    head = [t.clone() for t in net.resnet18.fc[0].parameters()]
    net.load_torchvision_state_dict(tv)
    got, want = net.resnet18.state_dict(), donor.resnet18.state_dict()
    for k in want:
        if not k.startswith("fc."):
            assert torch.equal(got[k], want[k]), k
    assert all(torch.equal(a, b) for a, b in zip(head, net.resnet18.fc[0].parameters()))
    del tv["layer3.0.downsample.1.running_var"]
    with pytest.raises(RuntimeError):
        net.load_torchvision_state_dict(tv)                 # the backbone loads strictly


@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (2, 3, 40, 56)])       # (the second: stages of 10 x 14, 5 x 7, 3 x 4, 2 x 2)
def test_cpu_forward_takes_the_plain_route(shape):
    net = _net().eval()
    x = torch.randn(*shape)
    with torch.no_grad():
        out = net(x)
        assert out.shape == (2, 128) and net.last_routes == ["plain"] * 20
        assert torch.equal(out, net.resnet18(x))
    net.train()
    out = net(x)
    assert out.shape == (2, 128) and out.requires_grad and net.last_routes == ["plain"] * 20


def test_optimized_canonicalizer_takes_the_network_on_the_cpu():
    """OptimizedGroupEquivariantImageCanonicalization(ResNet18Network(...), hp, (3, 64, 64)), C4, resize_shape = 32, B = 2.  The image
    action (orbit, canonicalize) has no CPU path in this package, as for the other canonicalizers, so the test goes up to the network's
    (G B, V) output on an orbit built with torch.rot90, and the loss computed from it."""
    import equiadapt_amd as ea

    net = _net()
    hp = types.SimpleNamespace(beta=1.0, input_crop_ratio=1.0, resize_shape=32, group_type="rotation", num_rotations=4,
                               artifact_err_wt=0.0, learn_ref_vec=False)
    can = ea.OptimizedGroupEquivariantImageCanonicalization(net, hp, (3, 64, 64)).eval()
    assert can.out_vector_size == 128 and can.num_group == 4 and can.reference_vector.shape == (1, 128)
    x = torch.nn.functional.interpolate(torch.randn(2, 3, 64, 64), size=32)
    orbit = torch.cat([torch.rot90(x, r, (2, 3)) for r in range(4)])
    with torch.no_grad():
        vec = can.canonicalization_network(orbit)
        assert vec.shape == (8, 128) and bool(torch.isfinite(vec).all())
        can.canonicalization_info_dict, can.device = {"vector_out": vec}, vec.device      # (what get_group_activations / canonicalize leave)
        assert bool(torch.isfinite(can.get_optimization_specific_loss()))


@pytest.mark.parametrize("cout,cin,k", [(128, 64, 3), (96, 32, 1)])
def test_pack_conv3x3_weights_layout(cout, cin, k):
    """Wpk[k dy + dx][s][n][b][32 h + i][t] = w[32 n + i][16 s + 8 b + 4 h + t][dy][dx], unpacked here index by index."""
    from equiadapt_amd import ops

    w = torch.randn(cout, cin, k, k)
    pk = ops.pack_conv3x3_weights(w)
    assert pk.shape == (k * k, cin // 16, cout // 32, 2, 64, 4) and pk.is_contiguous() and pk.dtype == torch.float32
    tap, s, n, b, lane, t = torch.meshgrid(*[torch.arange(d) for d in pk.shape], indexing="ij")
    h, i = lane // 32, lane % 32
    back = torch.zeros_like(w)
    back[32 * n + i, 16 * s + 8 * b + 4 * h + t, tap // k, tap % k] = pk
    assert torch.equal(back, w)
    for bad in (torch.randn(64, 64, 5, 5), torch.randn(64, 48, 3, 3), torch.randn(64, 64, 3)):
        with pytest.raises(ValueError):
            ops.pack_conv3x3_weights(bad)


def test_supported_query_on_the_edges_of_its_rule():
    from equiadapt_amd import _lib, ops

    _lib.build()
    lib = _lib.load()
    q = lib.eqa_conv3x3_supported
    assert q(4, 6, 6, 32, 32, 9, 1) and q(4, 6, 6, 512, 512, 9, 2) and q(4, 6, 6, 32, 512, 1, 2) and q(0, 6, 6, 64, 64, 9, 1)
    assert q(1, 1, 1, 64, 64, 9, 1) and q(1, 1, 1, 64, 64, 9, 2) and q(1, 1, 1, 64, 64, 1, 2)
    assert not q(4, 6, 6, 48, 64, 9, 1) and not q(4, 6, 6, 64, 48, 9, 1)            # off the multiples of 32
    assert not q(4, 6, 6, 544, 64, 9, 1) and not q(4, 6, 6, 64, 544, 9, 1)          # above 512
    assert not q(4, 6, 6, 16, 32, 9, 1) and not q(4, 6, 6, 32, 0, 9, 1)
    assert not q(4, 6, 6, 64, 64, 1, 1)                                             # the 1 x 1 form is the stride-2 shortcut only
    assert not q(4, 6, 6, 64, 64, 3, 1) and not q(4, 6, 6, 64, 64, 9, 3) and not q(4, 6, 6, 64, 64, 9, 0)
    assert not q(4, 0, 6, 64, 64, 9, 1) and not q(-1, 6, 6, 64, 64, 9, 1)
    # one 32-bit buffer range (0xffffff00 bytes) for x and for y: 2^16 pixels of 512 channels are 2^27 bytes per image
    assert q(31, 256, 256, 512, 512, 9, 1) and not q(32, 256, 256, 512, 512, 9, 1)
    assert q(31, 256, 256, 512, 32, 9, 1) and not q(32, 256, 256, 512, 32, 9, 1)    # x alone
    assert q(31, 256, 256, 32, 512, 9, 1) and not q(32, 256, 256, 32, 512, 9, 1)    # y alone
    assert not q(2 ** 40, 256, 256, 64, 64, 9, 1) and not q(1, 2 ** 20, 2 ** 20, 64, 64, 9, 1)
    assert ops.conv3x3_supported(4, 6, 6, 64, 128, 9, 2) and not ops.conv3x3_supported(4, 6, 6, 64, 128, 1, 1)


def test_launch_argument_checks_need_no_device():
    from equiadapt_amd import _lib, ops

    _lib.build()
    lib = _lib.load()
    shape = (2, 6, 6, 64, 64, 9, 1, None)
    # a refused shape is reported before any pointer is read
    assert lib.eqa_conv3x3_nhwc(None, None, None, None, 0, None, 2, 6, 6, 48, 64, 9, 1, None) == UNSUPPORTED
    assert lib.eqa_conv3x3_nhwc(None, None, None, None, 0, None, 2, 6, 6, 64, 64, 1, 1, None) == UNSUPPORTED
    assert lib.eqa_conv3x3_nhwc(None, None, None, None, 0, None, 32, 256, 256, 512, 512, 9, 1, None) == UNSUPPORTED
    assert lib.eqa_conv3x3_nhwc(None, None, None, None, 0, None, -1, 6, 6, 64, 64, 9, 1, None) == INVALID
    a, b, c, d = 4096, 8192, 12288, 16384                  # (never dereferenced: every call below is refused on its arguments)
    for args in ((None, b, c, None, 0, d), (a, None, c, None, 0, d), (a, b, None, None, 0, d), (a, b, c, None, 0, None)):
        assert lib.eqa_conv3x3_nhwc(*args, *shape) == INVALID, args
    assert lib.eqa_conv3x3_nhwc(a, b, c, None, 0, a, *shape) == INVALID          # y == x
    assert lib.eqa_conv3x3_nhwc(a, b, c, d, 1, d, *shape) == INVALID             # y == res
    assert lib.eqa_conv3x3_nhwc(a + 4, b, c, None, 0, d, *shape) == UNSUPPORTED  # off the 16-byte line
    assert lib.eqa_conv3x3_nhwc(None, None, None, None, 0, None, 0, 6, 6, 64, 64, 9, 1, None) == 0      # N = 0: nothing is launched
    with pytest.raises(RuntimeError, match="on the device"):
        ops.conv3x3_nhwc(torch.zeros(1, 4, 4, 32), torch.zeros(9, 2, 1, 2, 64, 4), torch.zeros(32))
