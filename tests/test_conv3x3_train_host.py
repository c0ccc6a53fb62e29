"""CPU-only: the data gradient's operand order (ops.pack_conv3x3_dgrad_weights) against its index formula and, through the data
gradient's own formula in fp64, against torch.nn.grad.conv2d_input; the new entry points declared, bound and linked alike; their
argument checks before any device work; ResNet18Network with the training switch on still plain on the CPU."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eqa_conv3x3_wgrad_supported", "eqa_conv3x3_wgrad_workspace_bytes", "eqa_conv3x3_wgrad", "eqa_conv3x3_dgrad_supported",
       "eqa_conv3x3_dgrad", "eqa_bn_res_act_fwd", "eqa_bn_res_act_bwd_reduce", "eqa_bn_res_act_bwd_apply")


def _unpack(wdpk, k):
    """The docstring's index formula, read backwards: U[tap][o][c] = the entry the kernel multiplies dz's channel o with for dx's c."""
    taps, S, NB = wdpk.shape[:3]
    tap, s, n, b, lane, t = torch.meshgrid(*[torch.arange(d) for d in wdpk.shape], indexing="ij")
    h, i = lane // 32, lane % 32
    U = torch.zeros(taps, 16 * S, 32 * NB, dtype=wdpk.dtype)
    U[tap, 16 * s + 8 * b + 4 * h + t, 32 * n + i] = wdpk
    return U


@pytest.mark.parametrize("cin,cout,taps,stride", [(ci, co, t, s) for (ci, co) in ((32, 96), (64, 64)) for t in (9, 1) for s in (1, 2)])
def test_dgrad_pack_is_its_index_formula_and_the_flip_and_transpose_convention_is_conv2d_input(cin, cout, taps, stride):
    from equiadapt_amd import ops

    k, pad = (3, 1) if taps == 9 else (1, 0)
    g = torch.Generator().manual_seed(100 * cin + cout + taps + stride)
    w = torch.randn(cout, cin, k, k, generator=g)
    wdpk = ops.pack_conv3x3_dgrad_weights(w)
    assert wdpk.shape == (taps, cout // 16, cin // 32, 2, 64, 4) and wdpk.is_contiguous()
    tap, s, n, b, lane, t = torch.meshgrid(*[torch.arange(d) for d in wdpk.shape], indexing="ij")
    h, i = lane // 32, lane % 32
    assert torch.equal(wdpk, w[16 * s + 8 * b + 4 * h + t, 32 * n + i, k - 1 - tap // k, k - 1 - tap % k])
    U = _unpack(wdpk, k).double()
    for H, W in ((5, 7), (6, 8)):
        OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        dz = torch.randn(2, OH, OW, cout, generator=g, dtype=torch.float64)
        dx = torch.zeros(2, H, W, cin, dtype=torch.float64)
        # the kernel's walk: tap (dy, dx) of input pixel (iy, ix) reads dz at ((iy + dy - pad) / s, (ix + dx - pad) / s) where both
        # divide and the quotients are inside
        for dy, dxx, iy, ix in itertools.product(range(k), range(k), range(H), range(W)):
            ty, tx = iy + dy - pad, ix + dxx - pad
            if ty < 0 or tx < 0 or ty % stride or tx % stride or ty // stride >= OH or tx // stride >= OW:
                continue
            dx[:, iy, ix, :] += dz[:, ty // stride, tx // stride, :] @ U[k * dy + dxx]
        want = torch.nn.grad.conv2d_input((2, cin, H, W), w.double(), dz.permute(0, 3, 1, 2), stride, pad).permute(0, 2, 3, 1)
        assert (dx - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), (H, W)


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
    assert os.path.join(_lib.CSRC, "conv3x3_train.hip") in _lib.SOURCES
    entry.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name


def test_queries_and_argument_checks_need_no_device():
    from equiadapt_amd import _lib

    _lib.build()
    lib = _lib.load()
    shapes = [(2, 5, 7, 64, 128, 9, 2), (1, 1, 1, 64, 64, 9, 1), (0, 4, 4, 512, 512, 9, 1), (2, 6, 8, 256, 512, 1, 2), (2, 4, 4, 48, 64, 9, 1),
              (2, 4, 4, 64, 544, 9, 1), (2, 4, 4, 64, 64, 1, 1), (2, 4, 4, 64, 64, 9, 3), (2 ** 20, 64, 64, 64, 64, 9, 1), (256, 24, 24, 64, 64, 9, 1)]
    for s in shapes:
        ok = lib.eqa_conv3x3_supported(*s)
        assert lib.eqa_conv3x3_wgrad_supported(*s) == ok and lib.eqa_conv3x3_dgrad_supported(*s) == ok, s
        assert (lib.eqa_conv3x3_wgrad_workspace_bytes(*s) > 0) == bool(ok and s[0]), s
    # the partial tiles: (splits, taps, Cout, Cin) floats, at most one split per wave of the chip's 1024
    assert lib.eqa_conv3x3_wgrad_workspace_bytes(1, 1, 1, 32, 32, 9, 1) == 9 * 32 * 32 * 4
    assert lib.eqa_conv3x3_wgrad_workspace_bytes(256, 24, 24, 64, 64, 9, 1) <= 1024 * 32 * 32 * 4 * 4
    assert lib.eqa_conv3x3_wgrad(None, None, None, None, 2, 4, 4, 48, 64, 9, 1, None) == -3      # refused before any pointer is read
    assert lib.eqa_conv3x3_wgrad(None, None, None, None, 2, 4, 4, 64, 64, 1, 1, None) == -3
    assert lib.eqa_conv3x3_wgrad(None, None, None, None, 2, 4, 4, 64, 64, 9, 1, None) == -1
    assert lib.eqa_conv3x3_wgrad(None, None, None, None, -1, 4, 4, 64, 64, 9, 1, None) == -1
    assert lib.eqa_conv3x3_dgrad(None, None, None, None, 2, 4, 4, 64, 544, 9, 1, None) == -3
    assert lib.eqa_conv3x3_dgrad(None, None, None, None, 2, 4, 4, 64, 64, 9, 1, None) == -1
    assert lib.eqa_conv3x3_dgrad(None, None, None, None, 0, 4, 4, 64, 64, 9, 1, None) == 0         # N = 0: nothing is launched
    assert lib.eqa_bn_res_act_fwd(None, None, None, None, 1, None, 0, 64, None) == 0
    assert lib.eqa_bn_res_act_fwd(None, None, None, None, 1, None, 8, 64, None) == -1
    assert lib.eqa_bn_res_act_bwd_reduce(*[None] * 5, 1, None, None, None, 8, 64, None) == -1
    assert lib.eqa_bn_res_act_bwd_apply(*[None] * 5, 1, *[None] * 7, 8, 64, None) == -1


def test_wrappers_raise_on_cpu_tensors():
    from equiadapt_amd import ops

    with pytest.raises(RuntimeError, match="on the device"):
        ops.conv3x3_wgrad(torch.zeros(1, 4, 4, 32), torch.zeros(1, 4, 4, 32))
    with pytest.raises(RuntimeError, match="on the device"):
        ops.conv3x3_dgrad(torch.zeros(1, 4, 4, 32), ops.pack_conv3x3_dgrad_weights(torch.zeros(32, 32, 3, 3)), (4, 4))
    with pytest.raises(RuntimeError):
        ops.bn_res_act_fwd(torch.zeros(8, 32), torch.zeros(32), torch.zeros(32), None, True)
    with pytest.raises(ValueError):
        ops.pack_conv3x3_dgrad_weights(torch.zeros(32, 48, 3, 3))


def test_training_switch_on_the_cpu_takes_the_plain_route(monkeypatch):
    import equiadapt_amd as ea

    monkeypatch.setenv("EQA_RESNET_TRAIN_KERNEL", "1")
    torch.manual_seed(0)
    net = ea.ResNet18Network((3, 32, 32), 1, 1, out_vector_size=8).train()
    assert net._train_applies(torch.zeros(2, 3, 32, 32)) is False
    out = net(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 8) and net.last_routes == ["plain"] * 20 and net.last_wgrad_routes == []
