"""CPU-only: WideResNet50Network / WideResNet101Network against the published layer plan (parameter, entry and convolution counts,
every key and shape, the stride on conv2, the published initialisation), their state-dict loaders, the plain route, the exports, and
eqa_convwide_*'s host-side queries and argument checks (admission table, K-split range and rule, workspace size) before any device
work."""
import math
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eqa_convwide_supported", "eqa_convwide_ksplit", "eqa_convwide_workspace_bytes", "eqa_convwide_nhwc")
BLOCKS = {"WideResNet50Network": (3, 4, 6, 3), "WideResNet101Network": (3, 4, 23, 3)}
# (parameters at 128 outputs, state-dict entries, convolutions)
FACTS = {"WideResNet50Network": (67_096_512, 320, 53), "WideResNet101Network": (125_099_968, 626, 104)}


def _plan(blocks, out_vector_size):
    """key -> shape from the published definition: stem 7 x 7 / 2 to 64; four layers of bottlenecks of planes 64, 128, 256, 512 with
    inner width 2 planes and 4 planes outputs; a projection in the first block of every layer; a Linear(2048, out) head."""
    def bn(prefix, c):
        return {prefix + ".weight": (c,), prefix + ".bias": (c,), prefix + ".running_mean": (c,), prefix + ".running_var": (c,),
                prefix + ".num_batches_tracked": ()}

    plan = {"conv1.weight": (64, 3, 7, 7), **bn("bn1", 64)}
    cin = 64
    for li, (planes, count) in enumerate(zip((64, 128, 256, 512), blocks)):
        width, cout = 2 * planes, 4 * planes
        for bi in range(count):
            p = f"layer{li + 1}.{bi}."
            plan[p + "conv1.weight"] = (width, cin, 1, 1)
            plan[p + "conv2.weight"] = (width, width, 3, 3)
            plan[p + "conv3.weight"] = (cout, width, 1, 1)
            plan.update(bn(p + "bn1", width))
            plan.update(bn(p + "bn2", width))
            plan.update(bn(p + "bn3", cout))
            if bi == 0:
                plan[p + "downsample.0.weight"] = (cout, cin, 1, 1)
                plan.update(bn(p + "downsample.1", cout))
            cin = cout
    plan["fc.0.weight"] = (out_vector_size, 2048)
    plan["fc.0.bias"] = (out_vector_size,)
    return plan


@pytest.fixture(scope="module")
def nets():
    import equiadapt_amd as ea

    torch.manual_seed(0)
    return {name: getattr(ea, name)((3, 32, 32), 1, 1) for name in BLOCKS}


def _forms(blocks, hw, batch):
    """(N, H, W, Cin, Cout, taps, stride) of every convolution behind the stem, for a map of hw x hw behind the stem's max-pool."""
    out, cin = [], 64
    for li, (planes, count) in enumerate(zip((64, 128, 256, 512), blocks)):
        width, cout = 2 * planes, 4 * planes
        for bi in range(count):
            stride = 2 if (bi == 0 and li > 0) else 1
            out.append((batch, hw, hw, cin, width, 1, 1))
            out.append((batch, hw, hw, width, width, 9, stride))
            if bi == 0:
                out.append((batch, hw, hw, cin, cout, 1, stride))
            hw = (hw - 1) // stride + 1
            out.append((batch, hw, hw, width, cout, 1, 1))
            cin = cout
    return out


@pytest.mark.parametrize("name", list(BLOCKS))
def test_counts_keys_and_shapes_are_the_published_plan(nets, name):
    net = nets[name]
    params, entries, convs = FACTS[name]
    sd = net.wideresnet.state_dict()
    assert sum(p.numel() for p in net.parameters()) == params
    assert len(sd) == entries
    assert sum(isinstance(m, nn.Conv2d) for m in net.modules()) == convs
    assert {k: tuple(v.shape) for k, v in sd.items()} == _plan(BLOCKS[name], 128)
    assert set(net.state_dict()) == {"wideresnet." + k for k in sd}
    assert tuple(sd["layer4.0.downsample.0.weight"].shape) == (2048, 1024, 1, 1)
    if name == "WideResNet101Network":
        assert tuple(sd["layer3.22.conv2.weight"].shape) == (512, 512, 3, 3)
    forms = {(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0]) for m in net.wideresnet.modules() if isinstance(m, nn.Conv2d)}
    forms.discard((3, 64, 7, 2))
    assert len(forms) == 23 and {(64, 128, 1, 1), (2048, 1024, 1, 1), (1024, 1024, 3, 2)} <= forms   # (24 with the stem)
    assert net.out_vector_size == 128 and not hasattr(net, "resnet18")


@pytest.mark.parametrize("name", list(BLOCKS))
def test_the_stride_sits_on_conv2(nets, name):
    w = nets[name].wideresnet
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(w, f"layer{li}")):
            want = (2, 2) if (bi == 0 and li > 1) else (1, 1)
            assert blk.conv1.stride == (1, 1) and blk.conv3.stride == (1, 1) and blk.conv2.stride == want, (li, bi)
            assert blk.conv2.padding == (1, 1) and blk.conv1.bias is None and blk.conv2.bias is None and blk.conv3.bias is None
            assert (blk.downsample is not None) == (bi == 0)
            if blk.downsample is not None:
                assert blk.downsample[0].stride == want and blk.downsample[0].kernel_size == (1, 1)


def test_initialisation_is_the_published_one(nets):
    w = nets["WideResNet50Network"].wideresnet
    checked = 0
    for m in w.modules():
        if isinstance(m, nn.Conv2d) and m.weight.numel() >= 10 ** 5:
            fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
            want = math.sqrt(2.0 / fan_out)
            assert abs(m.weight.std().item() - want) <= 0.05 * want, (m, m.weight.std().item(), want)
            assert abs(m.weight.mean().item()) <= 0.05 * want
            checked += 1
        elif isinstance(m, nn.BatchNorm2d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())
            assert bool((m.running_mean == 0).all()) and bool((m.running_var == 1).all())
    assert checked >= 30


def test_load_torchvision_state_dict_takes_the_backbone_and_leaves_the_head(nets):
    import equiadapt_amd as ea

    net = ea.WideResNet50Network((3, 32, 32), 1, 1, out_vector_size=16)
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.randn(s, generator=g) if k.split(".")[-1] != "num_batches_tracked" else torch.tensor(7))
          for k, s in _plan(BLOCKS["WideResNet50Network"], 16).items() if not k.startswith("fc.")}
    sd["fc.weight"] = torch.randn(1000, 2048, generator=g)
    sd["fc.bias"] = torch.randn(1000, generator=g)
    head = {k: v.clone() for k, v in net.wideresnet.fc.state_dict().items()}
    net.load_torchvision_state_dict(sd)
    got = net.wideresnet.state_dict()
    for k, v in sd.items():
        if not k.startswith("fc."):
            assert torch.equal(got[k], v), k
    for k, v in head.items():
        assert torch.equal(got["fc." + k], v), k
    missing = dict(sd)
    del missing["layer3.5.bn2.running_var"]
    with pytest.raises(RuntimeError, match="layer3.5.bn2.running_var"):
        net.load_torchvision_state_dict(missing)
    with pytest.raises(RuntimeError):
        ea.WideResNet101Network((3, 32, 32), 1, 1).load_torchvision_state_dict(sd)     # a 50's dict lacks the 101's blocks


def test_state_dict_round_trip(nets):
    import equiadapt_amd as ea

    src = nets["WideResNet50Network"]
    dst = ea.WideResNet50Network((3, 32, 32), 1, 1)
    dst.load_state_dict(src.state_dict(), strict=True)
    for (ka, va), (kb, vb) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def test_cpu_forward_is_the_plain_route(nets):
    net = nets["WideResNet50Network"].eval()
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y = net(x)
        assert y.shape == (1, 128) and net.last_routes == ["plain"] * 53 and net.last_ksplits == [0] * 53
        assert torch.equal(y, net.wideresnet(x))


def test_exports_resolve_from_all_three_packages():
    import equiadapt_amd as ea
    from equiadapt_amd import images
    from equiadapt_amd.images import WideResNet50Network, WideResNet101Network
    from equiadapt_amd.images import canonicalization_networks as cn
    from equiadapt_amd.images.canonicalization_networks import custom_nonequivariant_networks as mod

    for name, cls in (("WideResNet50Network", WideResNet50Network), ("WideResNet101Network", WideResNet101Network)):
        assert getattr(ea, name) is getattr(cn, name) is getattr(images, name) is getattr(mod, name) is cls
        assert name in ea.__all__


def test_new_symbols_are_declared_bound_and_linked():
    from equiadapt_amd import _lib
    import __graft_entry__ as entry

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eqa_hip.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/eqa_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
    assert int(re.search(r"#define\s+EQA_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 3
    assert os.path.join(_lib.CSRC, "conv_wide.hip") in _lib.SOURCES
    entry.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def lib():
    from equiadapt_amd import _lib

    _lib.build()
    return _lib.load()


def test_admission_table(lib):
    ok = lib.eqa_convwide_supported
    for taps in (1, 9):
        for stride in (1, 2):
            assert ok(2, 6, 8, 64, 96, taps, stride) == 1, (taps, stride)
            assert ok(2, 6, 8, 2048, 2048, taps, stride) == 1
    assert ok(2, 3, 3, 2048, 32, 9, 1) == 1 and ok(2, 3, 3, 32, 2048, 1, 1) == 1
    assert ok(0, 3, 3, 64, 64, 9, 1) == 1
    for bad in ((2, 3, 3, 2080, 64, 9, 1), (2, 3, 3, 64, 2080, 9, 1), (2, 3, 3, 48, 64, 9, 1), (2, 3, 3, 64, 48, 1, 1), (2, 3, 3, 0, 64, 9, 1),
                (2, 3, 3, 64, 64, 4, 1), (2, 3, 3, 64, 64, 9, 3), (2, 3, 3, 64, 64, 9, 0), (-1, 3, 3, 64, 64, 9, 1), (2, 0, 3, 64, 64, 9, 1)):
        assert ok(*bad) == 0, bad
    # the byte limit at its edge: x of 32 channels is 128 bytes a pixel, 0xffffff00 / 128 = 33554430 pixels
    edge = 0xFFFFFF00 // 128
    assert ok(1, 1, edge, 32, 32, 1, 1) == 1 and ok(1, 1, edge + 1, 32, 32, 1, 1) == 0
    assert ok(edge, 1, 1, 32, 32, 1, 1) == 1 and ok(edge + 1, 1, 1, 32, 32, 1, 1) == 0
    assert ok(1, 1, edge // 2, 32, 64, 1, 1) == 1 and ok(1, 1, edge // 2 + 1, 32, 64, 1, 1) == 0      # y is the larger map


@pytest.mark.parametrize("name", list(BLOCKS))
def test_the_chosen_split_stays_in_range_and_is_one_where_the_tiles_fill_the_chip(lib, name):
    seen_one = seen_more = False
    for batch in (1, 256):
        for form in _forms(BLOCKS[name], 24, batch):
            N, H, W, Cin, Cout, taps, stride = form
            assert lib.eqa_convwide_supported(*form) == 1, form
            ks = lib.eqa_convwide_ksplit(*form)
            half = taps * Cin // 32                       # T / 2
            assert 1 <= ks <= min(16, half), (form, ks)
            k, pad = (3, 1) if taps == 9 else (1, 0)
            P = N * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
            tiles = -(-P // 64) * (Cout // (64 if Cout % 64 == 0 else 32))
            if tiles >= 1024:
                assert ks == 1, (form, tiles, ks)
                seen_one = True
            else:
                # the smallest power of two that reaches 1024 units, inside the admitted range
                want = 1
                while want < 16 and tiles * want < 1024:
                    want *= 2
                assert ks == min(want, 16, half), (form, tiles, ks)
                seen_more = seen_more or ks > 1
            assert lib.eqa_convwide_workspace_bytes(*form, ks) == (0 if ks == 1 else ks * P * Cout * 4), form
            assert lib.eqa_convwide_workspace_bytes(*form, 0) == lib.eqa_convwide_workspace_bytes(*form, ks), form
    assert seen_one and seen_more


def test_workspace_size_and_refusals(lib):
    form = (2, 3, 3, 2048, 64, 1, 1)                      # P = 18, T / 2 = 64
    assert lib.eqa_convwide_workspace_bytes(*form, 1) == 0
    for ks in (2, 3, 5, 16):
        assert lib.eqa_convwide_workspace_bytes(*form, ks) == ks * 18 * 64 * 4
    assert lib.eqa_convwide_workspace_bytes(*form, 17) == 0 and lib.eqa_convwide_workspace_bytes(*form, -1) == 0
    assert lib.eqa_convwide_workspace_bytes(1, 2, 2, 32, 2048, 1, 1, 2) == 0        # T / 2 = 1: only ksplit 1 is admitted
    assert lib.eqa_convwide_ksplit(1, 2, 2, 32, 2048, 1, 1) == 1
    refused = (2, 3, 3, 2080, 64, 1, 1)
    assert lib.eqa_convwide_ksplit(*refused) == 0 and lib.eqa_convwide_workspace_bytes(*refused, 2) == 0
    assert lib.eqa_convwide_workspace_bytes(0, 3, 3, 2048, 64, 1, 1, 4) == 0        # N = 0: no pixels


def test_argument_checks_need_no_device(lib):
    call = lib.eqa_convwide_nhwc
    nul = [None] * 4
    assert call(*nul, 0, None, None, 2, 3, 3, 2080, 64, 9, 1, 1, None) == -3       # refused before any pointer is read
    assert call(*nul, 0, None, None, 2, 3, 3, 64, 64, 9, 3, 1, None) == -3
    assert call(*nul, 0, None, None, 2, 3, 3, 64, 64, 9, 1, 17, None) == -3        # ksplit out of range
    assert call(*nul, 0, None, None, 2, 3, 3, 64, 64, 1, 1, 3, None) == -3         # T / 2 = 2
    assert call(*nul, 0, None, None, 2, 3, 3, 64, 64, 9, 1, -1, None) == -3
    assert call(*nul, 0, None, None, 2, 3, 3, 64, 64, 9, 1, 1, None) == -1         # NULL operands
    assert call(*nul, 0, None, None, 2, 3, 3, 64, 64, 9, 1, 0, None) == -1
    assert call(*nul, 0, None, None, -1, 3, 3, 64, 64, 9, 1, 1, None) == -1
    assert call(*nul, 0, None, None, 0, 3, 3, 64, 64, 9, 1, 1, None) == 0          # N = 0: nothing is launched
    assert call(*nul, 0, None, None, 0, 3, 3, 64, 64, 9, 1, 4, None) == 0
    # (host addresses that are never read: the checks on values alone)
    x, w, b, r, y, ws = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    tail = (2, 3, 3, 64, 64, 9, 1)
    assert call(x, w, b, r, 0, y, None, *tail, 4, None) == -1                        # NULL workspace with ksplit > 1
    assert call(x, w, b, r, 0, x, ws, *tail, 4, None) == -1                          # y equal to x
    assert call(x, w, b, r, 0, r, ws, *tail, 1, None) == -1                          # y equal to res
    for alias in (x, w, b, r, y):
        assert call(x, w, b, r, 0, y, alias, *tail, 4, None) == -1, hex(alias)       # workspace equal to an operand
    assert call(x + 4, w, b, r, 0, y, ws, *tail, 4, None) == -3                      # unaligned pointers
    assert call(x, w, b, r + 8, 0, y, ws, *tail, 1, None) == -3
    assert call(x, w, b, r, 0, y, ws + 4, *tail, 4, None) == -3


def test_wrappers_raise_on_cpu_tensors_and_the_pack_is_general():
    from equiadapt_amd import ops

    wpk = ops.pack_conv3x3_weights(torch.zeros(2048, 1024, 1, 1))
    assert wpk.shape == (1, 64, 64, 2, 64, 4)
    w = torch.randn(64, 2048, 3, 3, generator=torch.Generator().manual_seed(5))
    wpk = ops.pack_conv3x3_weights(w)
    tap, s, n, b, lane, t = torch.meshgrid(*[torch.arange(d) for d in wpk.shape], indexing="ij")
    assert torch.equal(wpk, w[32 * n + lane % 32, 16 * s + 8 * b + 4 * (lane // 32) + t, tap // 3, tap % 3])
    with pytest.raises(RuntimeError, match="on the device"):
        ops.convwide_nhwc(torch.zeros(1, 4, 4, 32), ops.pack_conv3x3_weights(torch.zeros(32, 32, 3, 3)), torch.zeros(32))
