"""GPU: the FourierELU kernels (csrc/fourier_act.hip) against the fp64 CPU formula, ESCNNSteerableNetwork on the device against its
fp64 CPU plain-op evaluation, and SteerableImageCanonicalization end to end with that network."""
import copy
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd import _lib, ops
from equiadapt_amd.images.canonicalization_networks import steerable_networks as sn

pytestmark = pytest.mark.gpu

# (B, fields, H, W): 27 channels / 35 pixels, nothing a multiple of 4 or 64; 144-channel rows that straddle cache lines, several
# blocks (6992 fields of 256 per block); one pixel, one field per image
KERNEL_SHAPES = [(2, 3, 5, 7), (1, 16, 19, 23), (3, 1, 1, 1)]
IDX9 = [0, 1, 1, 2, 2, 3, 3, 4, 4]


def _kernel_case(shape, affine: bool, seed: int = 0):
    """x (channels-last fp32, CPU) with exact zeros, fields pushed below -20 at every sample (ELU's saturated branch) and entries
    of magnitude ~1e3; dy in [-1, 1]; scale in [0.5, 1.5], shift in [-1, 1] (or None)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = 2.0 * torch.randn(B, 9 * C, H, W, generator=g)
    xs = x.unflatten(1, (C, 9))
    pick = torch.rand(B, C, H, W, generator=g)
    xs[:, :, 0][pick < 0.15] -= 60.0                               # a_0 << -20: all 16 samples saturate (|other terms| < 40)
    big = (pick > 0.9)[:, :, None].expand_as(xs) & (torch.rand(xs.shape, generator=g) < 0.3)
    xs[big] = xs[big] * 500.0                                      # ~1e3
    xs[torch.rand(xs.shape, generator=g) < 0.1] = 0.0              # exact zeros
    x = xs.flatten(1, 2).contiguous(memory_format=torch.channels_last)
    dy = (2.0 * torch.rand(x.shape, generator=g) - 1.0).contiguous(memory_format=torch.channels_last)
    scale = 0.5 + torch.rand(C, 5, generator=g) if affine else None
    shift = 2.0 * torch.rand(C, generator=g) - 1.0 if affine else None
    return x, dy, scale, shift


def _formula(x, dy, scale, shift, dtype):
    """y = (A^T / 16) ELU(A (scale x + shift)) and dx by autograd, in plain torch ops at `dtype` on the CPU.  Returns (y, dx, u)."""
    C = x.shape[1] // 9
    x = x.to(dtype).contiguous().requires_grad_(True)
    u = x.unflatten(1, (C, 9))
    if scale is not None:
        u = u * scale.to(dtype)[:, IDX9][None, :, :, None, None]
        u = u + F.pad(shift.to(dtype)[:, None], (0, 8))[None, :, :, None, None]
    A = sn.sampling_matrix().to(dtype)
    y = torch.einsum("ij,bcihw->bcjhw", A / 16, F.elu(torch.einsum("ij,bcjhw->bcihw", A, u))).flatten(1, 2)
    (dx,) = torch.autograd.grad(y, x, dy.to(dtype))
    return y.detach(), dx, u.detach()


def _bound(u):
    """Per element 1e-5 * (1 + max |scale x + shift|), the maximum over the element's own field (its 9 coefficients): 25 fp32
    multiply-adds and one expf per output."""
    m = u.abs().amax(dim=2, keepdim=True).expand_as(u).flatten(1, 2)
    return 1e-5 * (1.0 + m)


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
@pytest.mark.parametrize("affine", [False, True])
def test_fourier_elu_kernels_match_the_fp64_formula(shape, affine):
    """Forward and backward, per element within 1e-5 * (1 + max |scale x + shift| over the element's field) of the fp64 CPU formula
    and its autograd.  The fp32 CPU plain-op path alone stays under half of that bound on these inputs: its largest error / bound
    is 0.025 (forward) and 0.010 (backward) -- asserted below, so the bound is not met by luck of one implementation.
    Two launches on the same input give the same bits."""
    dev = torch.device("cuda:0")
    x, dy, scale, shift = _kernel_case(shape, affine)
    y64, dx64, u = _formula(x, dy, scale, shift, torch.float64)
    bound = _bound(u)
    y32, dx32, _ = _formula(x, dy, scale, shift, torch.float32)
    r_fwd, r_bwd = float(((y32 - y64).abs() / bound).max()), float(((dx32 - dx64).abs() / bound).max())
    print(f"{shape} affine={affine}: fp32 CPU err / bound: fwd {r_fwd:.3f} bwd {r_bwd:.3f}")
    assert r_fwd < 0.5 and r_bwd < 0.5
    xd, dyd = x.to(dev), dy.to(dev)
    sd, hd = (scale.to(dev), shift.to(dev)) if affine else (None, None)
    assert xd.is_contiguous(memory_format=torch.channels_last)
    y = ops.fourier_elu(xd, sd, hd)
    dx = ops.fourier_elu_bwd(xd, dyd, sd, hd)
    assert y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
    k_fwd, k_bwd = float(((y.cpu() - y64).abs() / bound).max()), float(((dx.cpu() - dx64).abs() / bound).max())
    print(f"{shape} affine={affine}: kernel err / bound: fwd {k_fwd:.3f} bwd {k_bwd:.3f}")
    assert k_fwd <= 1.0 and k_bwd <= 1.0
    assert torch.equal(y, ops.fourier_elu(xd, sd, hd)) and torch.equal(dx, ops.fourier_elu_bwd(xd, dyd, sd, hd))
    assert torch.equal(xd.cpu(), x) and torch.equal(dyd.cpu(), dy)                      # inputs untouched


def test_fourier_elu_autograd_function_and_argument_checks():
    dev = torch.device("cuda:0")
    x, dy, _, _ = _kernel_case((2, 3, 5, 7), False, seed=1)
    y64, dx64, u = _formula(x, dy, None, None, torch.float64)
    xd = x.to(dev).requires_grad_(True)
    y = sn.FourierELUFunction.apply(xd)
    y.backward(dy.to(dev))
    assert float(((y.detach().cpu() - y64).abs() / _bound(u)).max()) <= 1.0
    assert float(((xd.grad.cpu() - dx64).abs() / _bound(u)).max()) <= 1.0
    # tensors that are not channels-last fp32 device tensors raise
    xc = x.to(dev)
    with pytest.raises(RuntimeError):
        ops.fourier_elu(x)                                                               # CPU
    with pytest.raises(RuntimeError):
        ops.fourier_elu(xc.contiguous())                                                 # NCHW
    with pytest.raises(RuntimeError):
        ops.fourier_elu(xc.double())
    with pytest.raises(ValueError):
        ops.fourier_elu(xc[:, :26].contiguous(memory_format=torch.channels_last))        # not a whole number of fields
    with pytest.raises(ValueError):
        ops.fourier_elu(xc, torch.ones(3, 4, device=dev), torch.zeros(3, device=dev))
    with pytest.raises(RuntimeError):
        ops.fourier_elu_bwd(xc, dy.to(dev).contiguous())
    # the C entry points: null pointers and zero sizes are errors, a misaligned map is unsupported
    lib = _lib.load()
    y = torch.empty_like(xc)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.eqa_fourier_elu_fwd(None, None, None, y.data_ptr(), 70, 3, st) == -1
    assert lib.eqa_fourier_elu_fwd(xc.data_ptr(), None, None, None, 70, 3, st) == -1
    assert lib.eqa_fourier_elu_fwd(xc.data_ptr(), None, None, y.data_ptr(), 0, 3, st) == -1
    assert lib.eqa_fourier_elu_fwd(xc.data_ptr(), None, None, y.data_ptr(), 70, 0, st) == -1
    assert lib.eqa_fourier_elu_bwd(xc.data_ptr(), None, None, None, y.data_ptr(), 70, 3, st) == -1
    assert lib.eqa_fourier_elu_bwd(xc.data_ptr(), None, None, y.data_ptr(), y.data_ptr(), -1, 3, st) == -1
    assert lib.eqa_fourier_elu_fwd(xc.data_ptr() + 4, None, None, y.data_ptr(), 60, 3, st) == -3


# ---------------------------------------------------------------------------------------------------------------------------------
# the network on the device


def _rel(a: torch.Tensor, ref: torch.Tensor) -> float:
    """max |a - ref| / max |ref|; a reference that is exactly zero (a weight slot that carries nothing) must be met exactly."""
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if not a.double().abs().max() > 0 else math.inf
    return float((a.double().cpu() - ref).abs().max()) / scale


def _turn(v: torch.Tensor, q: int) -> torch.Tensor:
    for _ in range(q % 4):
        v = torch.stack([-v[..., 1], v[..., 0]], dim=-1)
    return v


@functools.lru_cache(maxsize=None)
def _rgb_case():
    """The (3, 33, 33) network (4 fields, k = 7, 2 layers) with running statistics that are not the initial ones, a batch of two,
    and the eval outputs of the fp64 and fp32 CPU plain-op paths.  Shared, never modified."""
    torch.manual_seed(0)
    net = ea.ESCNNSteerableNetwork((3, 33, 33), 4, 7, "rotation", 2)
    with torch.no_grad():
        net.train()
        net(torch.randn(4, 3, 33, 33))
        for m in net.block:
            if isinstance(m, sn.FieldNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    net.eval()
    x = torch.randn(2, 3, 33, 33)
    with torch.no_grad():
        out64 = copy.deepcopy(net).double()(x.double())
        out32 = net(x)
    return net, x, out64, out32


def test_network_eval_matches_fp64_cpu_and_turns_with_the_input():
    """fp32 device network (HIP activation with the folded norm, cached banks, window-sum tail) against the fp64 CPU plain-op
    evaluation of the same weights: within 4 x the error of the fp32 CPU plain-op path against that same fp64 run (relative to
    max |out|).  Quarter-turn equivariance on the device: within twice that, by the triangle inequality.
    Measured on an MI355X: fp32 CPU 5.3e-7, device 1.7e-6 (tolerance 2.1e-6), equivariance 1.4e-6.  Layer by layer the device's
    errors are 1.0 - 1.4 x the CPU path's (convolutions 4.4e-7 / 1.0e-6 against 4.4e-7 / 8.3e-7 of the maps' largest entries); the
    output is a mean in which large terms cancel, so how much of a hidden map's error survives in it differs between two paths with
    equally good maps: the end-to-end ratio of 3 is that, not a weaker kernel."""
    dev = torch.device("cuda:0")
    net, x, out64, out32 = _rgb_case()
    tol = 4.0 * _rel(out32, out64)
    dnet = copy.deepcopy(net).to(dev).eval()
    with torch.no_grad():
        out = dnet(x.to(dev))
        err = _rel(out, out64)
        print(f"eval: fp32 CPU rel err {tol / 4:.2e}, device rel err {err:.2e}")
        assert out.shape == (2, 2, 2) and err <= tol
        assert torch.equal(out, dnet(x.to(dev)))                                          # cached banks, no atomics
        vmax = float(out64.norm(dim=-1).max())
        for q in (1, 2, 3):
            vq = dnet(torch.rot90(x, q, (-2, -1)).to(dev))
            e = float((vq.cpu().double() - _turn(out.cpu().double(), q)).norm(dim=-1).max()) / vmax
            print(f"eval: q={q} device equivariance rel err {e:.2e}")
            assert e <= 2.0 * tol
    # a changed weight is seen (the bank cache is keyed by the weight version)
    with torch.no_grad():
        dnet.block[0].weights.mul_(1.5)
        assert not torch.equal(out, dnet(x.to(dev)))


def test_network_training_step_matches_fp64_cpu():
    """One training step (batch statistics, autograd through FourierELUFunction and the window-sum tail): the output and every
    parameter gradient against the fp64 CPU plain-op path, each relative to its own largest entry, within 4 x the largest such
    error of the fp32 CPU plain-op path."""
    dev = torch.device("cuda:0")
    net, x, _, _ = _rgb_case()
    wgt = torch.tensor([[[0.7, -1.1], [0.4, 0.9]], [[-0.6, 0.8], [1.2, -0.3]]])

    def step(n, xx, w):
        n.train()
        n.zero_grad()
        out = n(xx)
        (out * w).sum().backward()
        return out.detach(), {name: p.grad.detach().clone() for name, p in n.named_parameters()}

    out64, g64 = step(copy.deepcopy(net).double(), x.double(), wgt.double())
    out32, g32 = step(copy.deepcopy(net), x, wgt)
    tol = 4.0 * max([_rel(out32, out64)] + [_rel(g32[k], g64[k]) for k in g64])
    dnet = copy.deepcopy(net).to(dev)
    out, g = step(dnet, x.to(dev), wgt.to(dev))
    errs = {"out": _rel(out, out64), **{k: _rel(g[k], g64[k]) for k in g64}}
    print(f"train: fp32 CPU largest rel err {tol / 4:.2e}; device: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert set(g) == set(g64) and all(torch.isfinite(v).all() for v in g.values())
    assert max(errs.values()) <= tol, errs
    # the running statistics moved like the CPU path's
    cnet = copy.deepcopy(net)
    step(cnet, x, wgt)
    for (name, b), (_, bc) in zip(dnet.named_buffers(), cnet.named_buffers()):
        if "running" in name:
            assert torch.allclose(b.cpu(), bc, rtol=1e-4, atol=1e-5), name


def test_network_hidden_layer_on_the_fft_convolution_route():
    """16 fields (144 channels), B = 8 on 33 x 33, k = 7, 2 layers: the smallest shape at which `fftconv.applicable_k` admits the
    hidden -> hidden convolution (8 tiles; its cost model prefers the FFT from 144 channels up), in eval (`conv_kxk`, cached
    spectra) and in a training step (`ConvKxKFunction`).  The same comparison and the same tolerance as the two tests above."""
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    net = ea.ESCNNSteerableNetwork((3, 33, 33), 16, 7, "rotation", 2)
    x = torch.randn(8, 3, 33, 33)
    with torch.no_grad():
        net.train()
        net(x)
    wgt = torch.randn(8, 2, 2)

    def step(n, xx, w):
        n.train()
        n.zero_grad()
        out = n(xx)
        (out * w).sum().backward()
        return out.detach(), {name: p.grad.detach().clone() for name, p in n.named_parameters()}

    def evaluate(n, xx):
        n.eval()
        with torch.no_grad():
            return n(xx)

    n64, n32, dnet = copy.deepcopy(net).double(), copy.deepcopy(net), copy.deepcopy(net).to(dev)
    e64 = evaluate(n64, x.double())
    tol = 4.0 * _rel(evaluate(n32, x), e64)
    with ops.KernelTimer() as t:
        got = evaluate(dnet, x.to(dev))
    assert "fft_gemm" in t.summary() and "fourier_elu" in t.summary(), t.summary()
    print(f"fft route eval: tolerance {tol:.2e}, device rel err {_rel(got, e64):.2e}")
    assert _rel(got, e64) <= tol
    assert torch.equal(got, evaluate(dnet, x.to(dev)))
    out64, g64 = step(n64, x.double(), wgt.double())
    out32, g32 = step(n32, x, wgt)
    tol = 4.0 * max([_rel(out32, out64)] + [_rel(g32[k], g64[k]) for k in g64])
    with ops.KernelTimer() as t:
        out, g = step(dnet, x.to(dev), wgt.to(dev))
    assert "fft_gemm" in t.summary(), t.summary()
    errs = {"out": _rel(out, out64), **{k: _rel(g[k], g64[k]) for k in g64}}
    print(f"fft route train: tolerance {tol:.2e}; device: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= tol, errs


# ---------------------------------------------------------------------------------------------------------------------------------
# SteerableImageCanonicalization end to end


def _smooth_images(B: int, C: int, H: int, seed: int) -> torch.Tensor:
    """Gaussian-blurred noise (sigma 2) times a radial window that is zero outside the inscribed disc."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * C, 1, H + 12, H + 12, generator=g)
    t = torch.arange(-6, 7, dtype=torch.float32)
    w = torch.exp(-t * t / 8.0)
    w = w / w.sum()
    x = F.conv2d(x, (w[:, None] * w[None, :])[None, None]).reshape(B, C, H, H)
    c = torch.arange(H, dtype=torch.float32) - (H - 1) / 2
    r = torch.sqrt(c[:, None] ** 2 + c[None, :] ** 2)
    return 10.0 * x * torch.clamp((H / 2 - 2 - r) / 4, 0, 1)


QUARTER = torch.tensor([[0.0, 1.0], [-1.0, 0.0]])      # R(v turned by +90 degrees) = R(v) @ QUARTER for R = [[c, s], [-s, c]]


def _matrix_tolerance(net, x_net: torch.Tensor) -> float:
    """delta for the unit vectors the matrices are made of: 2 x (4 x the fp32 CPU plain-op error against fp64, relative to the
    largest |v|) -- the device network's quarter-turn tolerance of the test above -- times max |v| / min |v|, since every
    sample's vector is normalised by its own length."""
    cnet = copy.deepcopy(net).cpu().eval()
    with torch.no_grad():
        v64 = copy.deepcopy(cnet).double()(x_net.double())
        v32 = cnet(x_net)
    n = v64[:, 0].norm(dim=-1)
    return 2.0 * 4.0 * _rel(v32, v64) * float(v64.norm(dim=-1).max() / n.min())


def test_steerable_canonicalization_gray_end_to_end():
    """(1, 33, 33), smooth input: the predicted matrices are rotations (1e-5); those of rot90(x, q) are those of x composed with
    the quarter turn in the sense that makes the canonical images of x and rot90(x, q) agree on the inscribed disc, within
    2 * delta * (H / 2) * max |grad x| (an angle error delta moves a sample by at most delta * H / 2 pixels)."""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = ea.ESCNNSteerableNetwork((1, 33, 33), 4, 7, "rotation", 2)
    with torch.no_grad():
        net.train()
        net(_smooth_images(4, 1, 33, seed=5))
    net.eval()
    hp = types.SimpleNamespace(input_crop_ratio=0.8, resize_shape=24)
    can = ea.SteerableImageCanonicalization(net, hp, (1, 33, 33)).to(dev).eval()
    x = _smooth_images(2, 1, 33, seed=6)
    delta = _matrix_tolerance(net, x)
    gy, gx = x[..., 1:, :-1] - x[..., :-1, :-1], x[..., :-1, 1:] - x[..., :-1, :-1]
    pix = 2.0 * delta * (33 / 2) * float(torch.sqrt(gx * gx + gy * gy).max())
    c = torch.arange(33, dtype=torch.float32) - 16
    disc = (torch.sqrt(c[:, None] ** 2 + c[None, :] ** 2) <= 16.0)
    with torch.no_grad():
        R = can.get_groupelement(x.to(dev))["rotation"].cpu()
        assert (R @ R.transpose(1, 2) - torch.eye(2)).abs().max() <= 1e-5 and (torch.linalg.det(R) - 1.0).abs().max() <= 1e-5
        y = can.canonicalize(x.to(dev)).cpu()
        assert y.shape == x.shape and float(y.abs().max()) > 0.1 * float(x.abs().max())
        for q in (1, 2, 3):
            xq = torch.rot90(x, q, (-2, -1)).to(dev)
            Rq = can.get_groupelement(xq)["rotation"].cpu()
            e = float((Rq - R @ torch.linalg.matrix_power(QUARTER, q)).abs().max())
            yq = can.canonicalize(xq).cpu()
            d = float(((yq - y).abs() * disc).max())
            print(f"gray q={q}: matrix err {e:.2e} (delta {delta:.2e}), canonical image err {d:.2e} (bound {pix:.2e})")
            assert e <= delta and d <= pix


def test_steerable_canonicalization_rgb_runs_and_trains():
    """(3, 32, 32), crop ratio 0.8, resize 24 (the tail takes the convolution + mean form: a 12 x 12 map under a 7 x 7 window):
    matrices quarter-turn-consistent, and a backward pass through canonicalize reaches every network parameter."""
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = ea.ESCNNSteerableNetwork((3, 24, 24), 4, 7, "rotation", 2)
    hp = types.SimpleNamespace(input_crop_ratio=0.8, resize_shape=24)
    can = ea.SteerableImageCanonicalization(net, hp, (3, 32, 32)).to(dev)
    x = _smooth_images(2, 3, 32, seed=7)
    can.train()
    with torch.no_grad():
        can.canonicalize(x.to(dev))                                 # running statistics
    can.eval()
    with torch.no_grad():
        x_net = can.transformations_before_canonicalization_network_forward(x.to(dev)).cpu()
        assert x_net.shape == (2, 3, 24, 24)
        delta = _matrix_tolerance(net, x_net)
        R = can.get_groupelement(x.to(dev))["rotation"].cpu()
        assert (R @ R.transpose(1, 2) - torch.eye(2)).abs().max() <= 1e-5
        for q in (1, 2, 3):
            Rq = can.get_groupelement(torch.rot90(x, q, (-2, -1)).to(dev))["rotation"].cpu()
            e = float((Rq - R @ torch.linalg.matrix_power(QUARTER, q)).abs().max())
            print(f"rgb q={q}: matrix err {e:.2e} (delta {delta:.2e})")
            assert e <= delta
    can.train()
    y = can.canonicalize(x.to(dev))
    assert y.shape == (2, 3, 32, 32)
    (y * torch.linspace(-1, 1, 32, device=dev)[None, None, :, None]).sum().backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert all(float(m.weights.grad.abs().max()) > 0 for m in net.block if isinstance(m, sn.SteerableConv))
