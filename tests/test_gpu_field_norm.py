"""GPU: the training-mode field norm on the kernels of csrc/field_norm.hip -- the statistics against fp64 sums, and
`FieldNormFourierELUFunction`, `FieldNorm.forward_elu` and an ESCNNSteerableNetwork training step against the fp64 CPU plain-op
path (`FieldNorm` + `FourierELU` modules, autograd).

Tolerance rule (that of tests/test_gpu_fourier_act.py): every tensor is measured relative to its own largest entry against the fp64
CPU result; the bound is 4 x the largest such error of the fp32 CPU plain-op path on the same inputs."""
import copy
import functools
import math
import types

import pytest
import torch

import equiadapt_amd as ea
from equiadapt_amd import _lib, ops
from equiadapt_amd.images.canonicalization_networks import steerable_networks as sn

pytestmark = pytest.mark.gpu

# (fields, B, H, W): 35 items, one block, a partial last 16-byte line; 3 does not divide 256, several tiles; the hidden map of the
# (3, 33, 33) network, several blocks; the configuration's field count; 5 fields (tiles of 240 items), many blocks
SHAPES = [(1, 1, 5, 7), (3, 2, 13, 13), (4, 2, 27, 27), (16, 2, 13, 13), (5, 3, 40, 40)]
FUNCTION_CASES = [(s, 0.7) for s in SHAPES] + [((3, 2, 13, 13), 30.0)]


def _map(shape, offset, seed=0):
    """x:(B, 9 fields, H, W) fp32 channels-last on the CPU: 2 N(0, 1), a_0 moved by `offset`."""
    C, B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(B, C, 9, H, W, generator=g)
    x[:, :, 0] += offset
    return x.flatten(1, 2).contiguous(memory_format=torch.channels_last)


def _rel(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def _norm(C, seed=1):
    torch.manual_seed(seed)
    norm = sn.FieldNorm(C)
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.5, 0.5)
    return norm.train()


def _plain(norm, x, dy, dtype):
    """FourierELU(FieldNorm(x)) and its gradients by autograd in plain torch ops at `dtype` on the CPU (a copy of `norm`, which also
    holds the moved running statistics afterwards)."""
    norm = copy.deepcopy(norm).to(dtype).train()
    act = sn.FourierELU(norm.fields).to(dtype)
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    y = act(norm(xx))
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "dx": xx.grad, "dweight": norm.weight.grad, "dbias": norm.bias.grad}, norm


@functools.lru_cache(maxsize=None)
def _function_case(shape, offset):
    """Inputs, the fp64 CPU results and the tolerance of the rule above.  Shared, never modified."""
    x = _map(shape, offset)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).contiguous(memory_format=torch.channels_last)
    norm = _norm(shape[0])
    r64, n64 = _plain(norm, x, dy, torch.float64)
    r32, _ = _plain(norm, x, dy, torch.float32)
    errs32 = {k: _rel(r32[k], r64[k]) for k in r64}
    return x, dy, norm, r64, n64, errs32


def _fp64_sums(x, C):
    xs = x.double().unflatten(1, (C, 9))
    a0 = xs[:, :, 0]
    sq = (xs[:, :, 1:] ** 2).unflatten(2, (4, 2)).sum(dim=(0, 3, 4, 5))
    sums = torch.cat([a0.sum(dim=(0, 2, 3))[:, None], (a0 * a0).sum(dim=(0, 2, 3))[:, None], sq], dim=1)
    mags = torch.cat([a0.abs().sum(dim=(0, 2, 3))[:, None], (a0 * a0).sum(dim=(0, 2, 3))[:, None], sq], dim=1)
    return sums, mags


@pytest.mark.parametrize("shape", SHAPES)
def test_statistics_are_fp64_sums_of_exact_terms(shape):
    """partial.sum(0) against fp64 torch sums of the same fp32 map, per entry within n 2^-52 sum |term| (fp64 summation of exact
    terms, n = pixels); `partial` has exactly eqa_field_norm_blocks rows and every one is written; two launches: the same bits."""
    dev = torch.device("cuda:0")
    C, B, H, W = shape
    x = _map(shape, 30.0)
    sums, mags = _fp64_sums(x, C)
    npix = B * H * W
    xd = x.to(dev)
    lib = _lib.load()
    blocks = lib.eqa_field_norm_blocks(npix, C)
    assert blocks >= 1
    partial = torch.full((blocks, C, 6), math.nan, dtype=torch.float64, device=dev)
    assert lib.eqa_field_norm_stats(xd.data_ptr(), partial.data_ptr(), npix, C, torch.cuda.current_stream().cuda_stream) == 0
    assert not torch.isnan(partial).any()
    got = ops.field_norm_stats(xd)
    assert got.shape == (blocks, C, 6) and got.dtype == torch.float64 and torch.equal(got, partial)
    err = (got.sum(0).cpu() - sums).abs()
    bound = npix * 2.0 ** -52 * mags
    print(f"{shape}: blocks {blocks}, largest err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(xd.cpu(), x)


def test_statistics_over_several_blocks_with_a_partial_last_one():
    """5 fields: tiles of 240 items.  On a map of ones sum a_0 counts the pixels of every (block, field): at least three blocks,
    every pixel counted once, and the last block holds fewer than the first."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    C, B = 5, 3
    found = None
    for H in range(40, 64):
        blocks = lib.eqa_field_norm_blocks(B * H * H, C)
        count = ops.field_norm_stats(torch.ones(B, 9 * C, H, H, device=dev).contiguous(memory_format=torch.channels_last))[:, :, 0]
        assert count.shape == (blocks, C) and (count.sum(0) == B * H * H).all()
        if blocks >= 3 and 0 < float(count[-1].sum()) < float(count[0].sum()):
            found = H
            break
    print(f"H = {found}: {blocks} blocks, items in the first / last block {float(count[0].sum())} / {float(count[-1].sum())}")
    assert found is not None


def _run_function(x, dy, norm, dev):
    dnorm = copy.deepcopy(norm).to(dev)
    xd = x.detach().to(dev).requires_grad_(True)
    y, mean, var = sn.FieldNormFourierELUFunction.apply(xd, dnorm.weight, dnorm.bias, dnorm.eps)
    assert not mean.requires_grad and not var.requires_grad
    y.backward(dy.to(dev))
    return {"y": y.detach(), "dx": xd.grad, "dweight": dnorm.weight.grad, "dbias": dnorm.bias.grad, "mean": mean, "var": var}


@pytest.mark.parametrize("shape,offset", FUNCTION_CASES)
def test_function_matches_fp64_cpu(shape, offset):
    """y, dx, dweight, dbias by the tolerance rule; the returned batch statistics to 1e-6 of the fp64 ones; two runs: the same
    bits.  (With a_0 + 30 the fp32 CPU path loses ~1e-5 to E[a_0^2] - mean^2, which makes the rule loose there: the apply
    kernel's a_0 - mean form has a test of its own below.)"""
    dev = torch.device("cuda:0")
    x, dy, norm, r64, _, errs32 = _function_case(shape, offset)
    tol = 4.0 * max(errs32.values())
    got = _run_function(x, dy, norm, dev)
    errs = {k: _rel(got[k], r64[k]) for k in r64}
    print(f"{shape} a_0 + {offset}: fp32 CPU " + ", ".join(f"{k} {v:.2e}" for k, v in errs32.items())
          + "; device " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert got["y"].is_contiguous(memory_format=torch.channels_last) and got["dx"].shape == x.shape
    assert max(errs.values()) <= tol, (errs, tol)
    sums, _ = _fp64_sums(x, shape[0])
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean64 = sums[:, 0] / n
    var64 = torch.cat([(sums[:, 1] / n - mean64 ** 2)[:, None], sums[:, 2:] / (2 * n)], dim=1)
    assert got["mean"].shape == (shape[0],) and got["var"].shape == (shape[0], 5)
    assert torch.allclose(got["mean"].double().cpu(), mean64, rtol=1e-6, atol=0.0)
    assert torch.allclose(got["var"].double().cpu(), var64, rtol=1e-6, atol=0.0)
    again = _run_function(x, dy, norm, dev)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_apply_kernel_subtracts_the_mean_before_it_scales():
    """3 fields, 2 x 13 x 13, dy on channel 0 of every field only.  dx_0 of the map with a_0 + 30, relative to its own largest
    entry, within 4 x the error of the fp32 CPU path on the map with a_0 + 0.7 and the same dy: the offset costs nothing."""
    dev = torch.device("cuda:0")
    shape = (3, 2, 13, 13)
    C = shape[0]
    dy = torch.zeros(2, C, 9, 13, 13)
    dy[:, :, 0] = torch.randn(2, C, 13, 13, generator=torch.Generator().manual_seed(11))
    dy = dy.flatten(1, 2).contiguous(memory_format=torch.channels_last)
    norm = _norm(C)

    def dx0(t):
        return t.unflatten(1, (C, 9))[:, :, 0]

    x_near = _map(shape, 0.7)
    r64, _ = _plain(norm, x_near, dy, torch.float64)
    r32, _ = _plain(norm, x_near, dy, torch.float32)
    tol = 4.0 * _rel(dx0(r32["dx"]), dx0(r64["dx"]))
    x_far = _map(shape, 30.0)
    f64, _ = _plain(norm, x_far, dy, torch.float64)
    f32, _ = _plain(norm, x_far, dy, torch.float32)
    got = _run_function(x_far, dy, norm, dev)
    err = _rel(dx0(got["dx"]), dx0(f64["dx"]))
    print(f"dx_0: fp32 CPU at a_0 + 0.7 {tol / 4:.2e} (tolerance {tol:.2e}), fp32 CPU at a_0 + 30 "
          f"{_rel(dx0(f32['dx']), dx0(f64['dx'])):.2e}, device at a_0 + 30 {err:.2e}")
    assert err <= tol


def test_module_moves_the_running_statistics_like_forward():
    """`FieldNorm.forward_elu` against `FieldNorm.forward` on the CPU: the same running statistics (rtol 1e-4, atol 1e-5) and batch
    count, with autograd and under no_grad (where it returns no graph); a constant a_0 map gives a finite y and finite gradients."""
    dev = torch.device("cuda:0")
    shape = (4, 2, 27, 27)
    x, dy, norm, r64, _, errs32 = _function_case(shape, 0.7)
    cnorm = copy.deepcopy(norm)
    dnorm = copy.deepcopy(norm).to(dev)
    for step, grad in enumerate((True, False), 1):
        with torch.set_grad_enabled(grad):
            cnorm(x)
            y = dnorm.forward_elu(x.to(dev))
        assert y.requires_grad == grad and (y.grad_fn is not None) == grad
        assert _rel(y, r64["y"]) <= 4.0 * max(errs32.values())
        assert int(dnorm.num_batches_tracked) == int(cnorm.num_batches_tracked) == step
        assert torch.allclose(dnorm.running_mean.cpu(), cnorm.running_mean, rtol=1e-4, atol=1e-5)
        assert torch.allclose(dnorm.running_var.cpu(), cnorm.running_var, rtol=1e-4, atol=1e-5)
    flat = x.clone()
    flat.unflatten(1, (4, 9))[:, :, 0] = torch.tensor([0.0, 0.1, -3.3, 30.0])[None, :, None, None]
    xd = flat.to(dev).requires_grad_(True)
    y = dnorm.forward_elu(xd)
    y.backward(dy.to(dev))
    for t in (y, xd.grad, dnorm.weight.grad, dnorm.bias.grad, dnorm.running_mean, dnorm.running_var):
        assert torch.isfinite(t).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the network


def _step(net, x, w, freeze_norms=False):
    net.train()
    if freeze_norms:
        for m in net.block:
            if isinstance(m, sn.FieldNorm):
                m.eval()
    net.zero_grad()
    out = net(x)
    (out * w).sum().backward()
    return {"out": out.detach(), **{name: p.grad.detach().clone() for name, p in net.named_parameters()}}


@functools.lru_cache(maxsize=None)
def _network_case():
    """The (3, 33, 33) network (4 fields, k = 7, 2 layers) with norm parameters and running statistics that are not the initial
    ones, a batch of two, and its training step on the fp64 / fp32 CPU plain-op paths, norms training and frozen.  Shared."""
    torch.manual_seed(0)
    net = ea.ESCNNSteerableNetwork((3, 33, 33), 4, 7, "rotation", 2)
    with torch.no_grad():
        net.train()
        net(torch.randn(4, 3, 33, 33))
        for m in net.block:
            if isinstance(m, sn.FieldNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, 3, 33, 33)
    w = torch.tensor([[[0.7, -1.1], [0.4, 0.9]], [[-0.6, 0.8], [1.2, -0.3]]])
    ref, tol = {}, {}
    for frozen in (False, True):
        g64 = _step(copy.deepcopy(net).double(), x.double(), w.double(), frozen)
        g32 = _step(copy.deepcopy(net), x, w, frozen)
        ref[frozen], tol[frozen] = g64, 4.0 * max(_network_errs(g32, g64).values())
    return net, x, w, ref, tol


def _network_errs(g, g64):
    """Relative to each tensor's largest entry; a reference that is exactly zero (a weight slot that carries nothing) must be met
    exactly."""
    errs = {}
    for k, r in g64.items():
        if float(r.abs().max()) == 0.0:
            errs[k] = 0.0 if float(g[k].abs().max()) == 0.0 else math.inf
        else:
            errs[k] = _rel(g[k], r)
    return errs


FIELD_NORM_LAUNCHES = {"field_norm_stats", "field_norm_elu_bwd_reduce", "field_norm_elu_bwd_apply"}


def test_network_training_step_runs_the_field_norm_kernels(monkeypatch):
    """One training step under `ops.KernelTimer`: the three field-norm launches are in it; with EQA_FIELD_NORM_KERNEL=0 none of
    them is; both steps meet the tolerance rule against the fp64 CPU step."""
    dev = torch.device("cuda:0")
    net, x, w, ref, tol = _network_case()
    for knob, present in (("1", True), ("0", False)):
        monkeypatch.setenv("EQA_FIELD_NORM_KERNEL", knob)
        dnet = copy.deepcopy(net).to(dev)
        with ops.KernelTimer() as t:
            g = _step(dnet, x.to(dev), w.to(dev))
        names = set(t.summary())
        assert (FIELD_NORM_LAUNCHES <= names) if present else not (FIELD_NORM_LAUNCHES & names), names
        assert "fourier_elu" in names
        errs = _network_errs(g, ref[False])
        print(f"EQA_FIELD_NORM_KERNEL={knob}: tolerance {tol[False]:.2e}; device largest rel err {max(errs.values()):.2e}")
        assert set(g) == set(ref[False]) and max(errs.values()) <= tol[False], errs


def test_network_with_frozen_norms_keeps_the_folded_route():
    """Norms in eval() while the rest trains: no batch statistics, so no field-norm launch, and the step still matches."""
    dev = torch.device("cuda:0")
    net, x, w, ref, tol = _network_case()
    dnet = copy.deepcopy(net).to(dev)
    before = {k: v.clone() for k, v in dnet.named_buffers() if "running" in k}
    with ops.KernelTimer() as t:
        g = _step(dnet, x.to(dev), w.to(dev), freeze_norms=True)
    names = set(t.summary())
    assert not (FIELD_NORM_LAUNCHES & names) and "fourier_elu" in names and "fourier_elu_bwd" in names, names
    errs = _network_errs(g, ref[True])
    print(f"frozen norms: tolerance {tol[True]:.2e}; device largest rel err {max(errs.values()):.2e}")
    assert max(errs.values()) <= tol[True], errs
    assert all(torch.equal(v, dict(dnet.named_buffers())[k]) for k, v in before.items())


def test_route_predicate(monkeypatch):
    """The fused route is taken by a training norm with at most FIELD_NORM_MAX_FIELDS fields and both knobs on, by nothing else."""
    monkeypatch.delenv("EQA_FIELD_NORM_KERNEL", raising=False)
    monkeypatch.delenv("EQA_FOURIER_KERNEL", raising=False)
    ok = types.SimpleNamespace(training=True, fields=ops.FIELD_NORM_MAX_FIELDS)
    assert sn.fused_field_norm(ok)
    assert not sn.fused_field_norm(types.SimpleNamespace(training=True, fields=ops.FIELD_NORM_MAX_FIELDS + 1))
    assert not sn.fused_field_norm(types.SimpleNamespace(training=False, fields=4))
    monkeypatch.setenv("EQA_FIELD_NORM_KERNEL", "0")
    assert not sn.fused_field_norm(ok)
    monkeypatch.setenv("EQA_FIELD_NORM_KERNEL", "1")
    monkeypatch.setenv("EQA_FOURIER_KERNEL", "0")
    assert not sn.fused_field_norm(ok)


def test_entry_points_refuse_before_they_launch():
    """More fields than the kernels take: unsupported, from NULL pointers too; NULL maps and npix <= 0: invalid; a map off its
    16-byte line: unsupported.  None of these launches anything."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    F = lib.eqa_field_norm_max_fields()
    assert F == ops.FIELD_NORM_MAX_FIELDS
    assert lib.eqa_field_norm_blocks(70, F + 1) <= 0 and lib.eqa_field_norm_blocks(0, 3) <= 0 and lib.eqa_field_norm_blocks(70, 0) <= 0
    assert lib.eqa_field_norm_blocks(70, F) >= 1
    assert lib.eqa_field_norm_stats(None, None, 70, F + 1, st) == -3
    assert lib.eqa_field_norm_elu_bwd_reduce(None, None, None, None, None, 70, F + 1, st) == -3
    assert lib.eqa_field_norm_elu_bwd_apply(None, None, None, None, None, None, 70, F + 1, st) == -3
    x = torch.zeros(2, 27, 5, 7, device=dev).contiguous(memory_format=torch.channels_last)
    dy, dx = torch.zeros_like(x), torch.full_like(x, 5.0)
    scale, shift, coef = torch.ones(3, 5, device=dev), torch.zeros(3, device=dev), torch.zeros(3, 7, device=dev)
    part = torch.full((lib.eqa_field_norm_blocks(70, 3), 3, 6), 5.0, dtype=torch.float64, device=dev)
    px, pg, pd, ps, ph, pc, pp = (t.data_ptr() for t in (x, dy, dx, scale, shift, coef, part))
    assert lib.eqa_field_norm_stats(None, pp, 70, 3, st) == -1
    assert lib.eqa_field_norm_stats(px, None, 70, 3, st) == -1
    assert lib.eqa_field_norm_stats(px, pp, 0, 3, st) == -1
    assert lib.eqa_field_norm_stats(px, pp, 70, 0, st) == -1
    assert lib.eqa_field_norm_stats(px + 4, pp, 60, 3, st) == -3
    assert lib.eqa_field_norm_elu_bwd_reduce(None, ps, ph, pg, pp, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_reduce(px, ps, ph, None, pp, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_reduce(px, ps, ph, pg, None, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_reduce(px, ps, ph, pg, pp, -1, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_reduce(px, ps, ph, pg + 4, pp, 60, 3, st) == -3
    assert lib.eqa_field_norm_elu_bwd_apply(None, ps, ph, pg, pc, pd, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_apply(px, ps, ph, None, pc, pd, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_apply(px, ps, ph, pg, None, pd, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_apply(px, ps, ph, pg, pc, None, 70, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_apply(px, ps, ph, pg, pc, pd, 0, 3, st) == -1
    assert lib.eqa_field_norm_elu_bwd_apply(px, ps, ph, pg, pc, pd + 4, 60, 3, st) == -3
    torch.cuda.synchronize()
    assert (dx == 5.0).all() and (part == 5.0).all()                                     # nothing ran
    with pytest.raises(RuntimeError):
        ops.field_norm_stats(x.contiguous())                                            # NCHW
    with pytest.raises(ValueError):
        ops.field_norm_elu_bwd_apply(x, dy, scale, shift, coef[:, :6])
    with pytest.raises(_lib.EqaLibraryError):
        ops.field_norm_stats(torch.zeros(1, 9 * (F + 1), 2, 2, device=dev).contiguous(memory_format=torch.channels_last))
