"""CPU: the host half of the training-mode field norm on the kernels -- `field_norm_scale_shift` and
`field_norm_backward_coefficients` (steerable_networks.py) fed fp64 torch sums -- against autograd through the plain-op
`FourierELU(FieldNorm(x))` in fp64."""
import pytest
import torch

from equiadapt_amd.images.canonicalization_networks import steerable_networks as sn

IDX9 = [0, 1, 1, 2, 2, 3, 3, 4, 4]
SHAPES = [(1, 1, 5, 7), (3, 2, 13, 13), (4, 2, 27, 27)]          # (fields, B, H, W)


def _modules(C, seed):
    torch.manual_seed(seed)
    norm, act = sn.FieldNorm(C).double().train(), sn.FourierELU(C).double()
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.5, 0.5)
    return norm, act


def _forward_sums(x, C):
    xs = x.unflatten(1, (C, 9))
    sq = (xs[:, :, 1:] ** 2).unflatten(2, (4, 2)).sum(dim=(0, 3, 4, 5))
    return torch.cat([xs[:, :, 0].sum(dim=(0, 2, 3))[:, None], (xs[:, :, 0] ** 2).sum(dim=(0, 2, 3))[:, None], sq], dim=1)


def _closed_form(x, dy, norm, act):
    """(y, dx, dweight, dbias, mean, var) of FourierELU(FieldNorm(x)) from the two finalisation functions and the sums they take;
    du, the activation's own gradient at u, comes from autograd through `act` alone."""
    C = norm.fields
    n = x.shape[0] * x.shape[2] * x.shape[3]
    w, b = norm.weight.detach(), norm.bias.detach()
    mean, var, scale, shift = sn.field_norm_scale_shift(_forward_sums(x, C), n, w, b, norm.eps, dtype=torch.float64)
    xs = x.unflatten(1, (C, 9))
    u = xs * scale[:, IDX9][None, :, :, None, None]
    u[:, :, 0] += shift[None, :, None, None]
    u = u.flatten(1, 2).requires_grad_(True)
    y = act(u)
    (du,) = torch.autograd.grad(y, u, dy)
    dus = du.unflatten(1, (C, 9))
    T = (dus[:, :, 1:] * xs[:, :, 1:]).unflatten(2, (4, 2)).sum(dim=(0, 3, 4, 5))
    bsums = torch.cat([dus[:, :, 0].sum(dim=(0, 2, 3))[:, None], (dus[:, :, 0] * xs[:, :, 0]).sum(dim=(0, 2, 3))[:, None], T], dim=1)
    coef, dweight, dbias = sn.field_norm_backward_coefficients(bsums, w, mean, var, n, norm.eps)
    assert coef.shape == (C, 7) and dweight.shape == (C, 5) and dbias.shape == (C,)
    k0, mu, c = coef[:, 0], coef[:, 1], coef[:, 2:]
    dx = dus * scale[:, IDX9][None, :, :, None, None] - xs * c[:, IDX9][None, :, :, None, None]
    dx[:, :, 0] = (scale[:, 0][None, :, None, None] * dus[:, :, 0] - k0[None, :, None, None]
                   - c[:, 0][None, :, None, None] * (xs[:, :, 0] - mu[None, :, None, None]))
    return y.detach(), dx.flatten(1, 2), dweight, dbias, mean, var


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_matches_fp64_autograd(shape):
    """y, dx, dweight, dbias within 1e-12 of autograd, each relative to its own largest entry (measured: 3e-16); the statistics are
    those `FieldNorm.forward` moves its running averages by."""
    C, B, H, W = shape
    norm, act = _modules(C, seed=1)
    x = (2.0 * torch.randn(B, 9 * C, H, W, dtype=torch.float64) + 0.7).requires_grad_(True)
    dy = torch.randn(B, 9 * C, H, W, dtype=torch.float64)
    y_ref = act(norm(x))
    y_ref.backward(dy)
    y, dx, dweight, dbias, mean, var = _closed_form(x.detach(), dy, norm, act)
    errs = {"y": _rel(y, y_ref.detach()), "dx": _rel(dx, x.grad), "dweight": _rel(dweight, norm.weight.grad),
            "dbias": _rel(dbias, norm.bias.grad)}
    print(shape, errs)
    assert max(errs.values()) <= 1e-12, errs
    n = B * H * W
    unbiased = torch.cat([var[:, :1] * (n / max(n - 1, 1)), var[:, 1:]], dim=1)
    assert torch.allclose(norm.running_mean, 0.1 * mean, rtol=1e-12, atol=1e-14)
    assert torch.allclose(norm.running_var, 0.9 + 0.1 * unbiased, rtol=1e-12, atol=1e-14)


def test_fp32_tables_are_the_rounded_fp64_ones():
    """The default output type rounds once: scale is the rounded fp64 scale, and the shift is formed from that rounded scale."""
    C, B, H, W = 3, 2, 13, 13
    norm, _ = _modules(C, seed=2)
    x = 2.0 * torch.randn(B, 9 * C, H, W, dtype=torch.float64) + 30.0
    n, w, b = B * H * W, norm.weight.detach(), norm.bias.detach()
    sums = _forward_sums(x, C)
    mean, var, scale, shift = sn.field_norm_scale_shift(sums, n, w, b, norm.eps)
    _, _, scale64, _ = sn.field_norm_scale_shift(sums, n, w, b, norm.eps, dtype=torch.float64)
    assert mean.dtype == var.dtype == torch.float64 and scale.dtype == shift.dtype == torch.float32
    assert torch.equal(scale, scale64.float())
    assert torch.equal(shift, (b - mean * scale[:, 0].double()).float())


def test_constant_a0_map_gives_finite_tables():
    """var_0 = 0 (and, here, a sum of squares that rounds below n mean^2: the clamp): scale, shift and coefficients are finite, and
    the closed form still matches autograd."""
    C, B, H, W = 3, 2, 13, 13
    norm, act = _modules(C, seed=3)
    x = torch.randn(B, 9 * C, H, W, dtype=torch.float64)
    x.unflatten(1, (C, 9))[:, :, 0] = torch.tensor([0.1, -3.3, 30.0], dtype=torch.float64)[None, :, None, None]
    dy = torch.randn(B, 9 * C, H, W, dtype=torch.float64)
    y, dx, dweight, dbias, mean, var = _closed_form(x, dy, norm, act)
    assert float(var[:, 0].max()) <= 1e-12 and float(var[:, 0].min()) >= 0.0
    for t in (y, dx, dweight, dbias, mean, var):
        assert torch.isfinite(t).all()
    xr = x.clone().requires_grad_(True)
    act(norm(xr)).backward(dy)
    assert _rel(y, act(norm(x)).detach()) <= 1e-9 and _rel(dbias, norm.bias.grad) <= 1e-9
    assert torch.isfinite(xr.grad).all() and _rel(dx, xr.grad) <= 1e-6
