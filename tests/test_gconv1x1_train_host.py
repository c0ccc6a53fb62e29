"""CPU-only: the entry points of the 1 x 1 convolution's filter gradient are declared and bound alike, their argument checks run
before any device work, and ESCNNWRNEquivariantNetwork in training mode on the CPU still takes the plain route."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eqa_gconv1x1_wgrad_supported", "eqa_gconv1x1_wgrad_workspace_bytes", "eqa_gconv1x1_wgrad")


def test_new_symbols_are_declared_and_bound_with_matching_argument_counts():
    from equiadapt_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eqa_hip.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/eqa_hip.h"
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")), name
    assert int(re.search(r"#define\s+EQA_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 3


def test_queries_and_argument_checks_need_no_device():
    from equiadapt_amd import _lib

    _lib.build()
    lib = _lib.load()
    for sizes in ((100, 32, 32), (2 ** 21 - 1, 64, 512), (0, 512, 512), (100, 48, 64), (100, 64, 544), (2 ** 21, 64, 512), (100, 16, 32)):
        assert lib.eqa_gconv1x1_wgrad_supported(*sizes) == lib.eqa_gconv1x1_supported(*sizes), sizes
        assert (lib.eqa_gconv1x1_wgrad_workspace_bytes(*sizes) > 0) == bool(sizes[0] and lib.eqa_gconv1x1_supported(*sizes)), sizes
    # the partial tiles: (splits, Cin + 1, Cout) floats, at most one split per wave of the chip's 1024
    assert lib.eqa_gconv1x1_wgrad_workspace_bytes(1, 32, 32) == 33 * 32 * 4
    assert lib.eqa_gconv1x1_wgrad_workspace_bytes(8 * 108 * 108, 256, 256) <= 256 * 257 * 256 * 4
    assert lib.eqa_gconv1x1_wgrad(None, None, None, None, None, 100, 48, 64, None) == -3       # refused before any pointer is read
    assert lib.eqa_gconv1x1_wgrad(None, None, None, None, None, 100, 64, 64, None) == -1
    assert lib.eqa_gconv1x1_wgrad(None, None, None, None, None, -1, 64, 64, None) == -1


def test_wgrad_raises_on_cpu_tensors():
    from equiadapt_amd import ops

    with pytest.raises(RuntimeError, match="on the device"):
        ops.gconv1x1_wgrad(torch.zeros(8, 32), torch.zeros(8, 32))


def test_training_on_the_cpu_takes_the_plain_route():
    """kernel_size = 1, fp64 (the host has no fp32 group pooling): train() on the CPU is the plain route -- wide enough (32 to 256
    channels) that every bottleneck 1 x 1 layer would be on the kernels on the device --, equal to the module sequence evaluated
    layer by layer + the mean, with a gradient for every parameter and the running statistics updated."""
    import copy

    import equiadapt_amd as ea

    torch.manual_seed(3)
    net = ea.ESCNNWRNEquivariantNetwork((3, 9, 9), 32, 1, "rotation", 6, 4).double().train()
    x = torch.randn(2, 3, 9, 9, dtype=torch.float64)
    ref = copy.deepcopy(net)
    out = net(x)
    assert set(net.last_routes) == {"conv2d"} and len(net.last_routes) == 17
    out.sum().backward()
    want = torch.mean(ref.eqv_network(x), dim=(1, 3, 4))
    want.sum().backward()
    assert out.shape == (2, 4) and (out - want).abs().max().item() <= 1e-12
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert (p.grad - q.grad).abs().max().item() <= 1e-10 * max(1.0, q.grad.abs().max().item()), n
    for (n, b), c in zip(net.named_buffers(), ref.buffers()):
        assert torch.allclose(b, c, rtol=0, atol=1e-12), n
    assert int(net.eqv_network[1].num_batches_tracked) == 1
