"""ESCNNSteerableNetwork: SO(2)-steerable canonicalization network that outputs two rotation-equivariant 2-vectors per image.

Reference: equiadapt/images/canonicalization_networks/escnn_networks.py:120-224, built there from e2cnn ``R2Conv`` over
``Rot2dOnR2(N=-1)``, ``GNormBatchNorm`` and ``FourierELU(irreps 0..4, N=16)``; it is the network the reference pairs with
``SteerableImageCanonicalization`` (``canonicalization_type: steerable``).

e2cnn is not available to this build and its basis is NOT restated here.  This class keeps the reference's constructor, layer
order (``[conv k x k, no padding, no bias -> field norm -> FourierELU] x num_layers -> conv k x k -> 2 x irrep(1) -> spatial
mean``) and output contract ((B, 2, 2): row i = (Re, Im) of output field i), with a parameterisation of its own.  IT IS A
DIFFERENT FUNCTION CLASS: weights trained with e2cnn cannot be loaded, and the equivariance is exact for quarter turns only
(square pixel grid, Gaussian rings); the error at other angles is measured by tools/steerable_equivariance.py and tabulated in
DESIGN.md.

Fields.  A hidden map with C fields has 9 C channels; channel 9 c + j is coefficient j of field c: j = 0 -> a_0, j = 2m-1 / 2m ->
Re / Im c_m for m = 1..4.  The field describes f(phi) = a_0 + sum_m sqrt(2) (Re c_m cos m phi + Im c_m sin m phi); a rotation by t
maps c_m to e^{imt} c_m.  The input is frequency 0 only, the output frequency 1 only (two fields, four channels).

Steerable convolution, frequency n -> m, in complex form:  c_m(x) = sum_y [ kappa_mn(y) c_n(x+y) + kappa'_mn(y) conj(c_n(x+y)) ],
kappa_mn(r, phi) = sum_j w_j R_j(r) e^{i(m-n)phi}, kappa' the same with harmonic m+n and weights of its own (m, n > 0 only); m = 0
keeps the real part.  Rings R_j(r) = exp(-(r-j)^2 / (2 0.6^2)), j = 0..k//2, masked to r <= k/2; ring j carries the harmonics
|d| <= 2j; THE CENTRE TAP IS ZERO FOR EVERY HARMONIC d != 0 (rings j >= 1 spill ~0.25 onto r = 0, a fixed point of the rotation:
left in, quarter-turn equivariance is lost at the 3 % level).
"""
import math
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from equiadapt_amd import ops
from equiadapt_amd.common.derived import DerivedCache, refuse_e2cnn_state_dict
from equiadapt_amd.images.canonicalization_networks import fftconv
from equiadapt_amd.images.canonicalization_networks.pooling import WindowSumsFunction

MAX_FREQ = 4                        # hidden fields hold frequencies 0..4 (the reference's FourierELU irreps)
FIELD_DIM = 2 * MAX_FREQ + 1        # 9 == ops.FOURIER_FIELD_DIM
NUM_SAMPLES = 16                    # FourierELU's sampling grid (the reference's N = 16)
RING_SIGMA = 0.6
# phi = atan2(PHI_SIGN * row, col).  With -1 (row axis up) the network turns its vectors with torch.rot90, v(rot90(x, q)) =
# e^{+iq pi/2} v(x), which is the sense in which SteerableImageCanonicalization undoes the rotation (the canonical images of x and
# rot90(x, q) then agree: tests/test_gpu_fourier_act.py); with +1 the vectors turn the other way and it would double the rotation.
PHI_SIGN = -1.0

_FREQS = {"scalar": (0,), "fourier": tuple(range(MAX_FREQ + 1)), "vector": (1,)}
_FOURIER_ACT_KERNEL = "EQA_FOURIER_KERNEL"     # "0": the op-by-op activation on the device as well (A/B timing, tools/kbench_fourier_act.py)
_FIELD_NORM_KERNEL = "EQA_FIELD_NORM_KERNEL"   # "0": training keeps the norm in torch ops in front of FourierELUFunction (tools/kbench_field_norm.py)
_STEER_LIFT_KERNEL = "EQA_STEER_LIFT_KERNEL"   # "0": the first layer stays the library's convolution (A/B timing, tools/kbench_steer_lift.py)


def sampling_matrix() -> torch.Tensor:
    """A:(16, 9) fp64, the field's values at phi_i = 2 pi i / 16: A[i, 0] = 1, A[i, 2m-1] = sqrt2 cos m phi_i, A[i, 2m] = sqrt2 sin m phi_i.
    A^T A = 16 I: the activation is y = (A^T / 16) ELU(A x)."""
    phi = 2.0 * math.pi * torch.arange(NUM_SAMPLES, dtype=torch.float64) / NUM_SAMPLES
    A = torch.ones(NUM_SAMPLES, FIELD_DIM, dtype=torch.float64)
    for m in range(1, MAX_FREQ + 1):
        A[:, 2 * m - 1] = math.sqrt(2.0) * torch.cos(m * phi)
        A[:, 2 * m] = math.sqrt(2.0) * torch.sin(m * phi)
    return A


def steerable_basis(k: int) -> torch.Tensor:
    """(17, k//2 + 1, k, k, 2) fp64: entry [d + 8, j] = R_j(r) (cos d phi, sin d phi) for the harmonics d = -8..8 (m - n and m + n of
    frequencies up to 4) and the rings j, zero where ring j does not carry d (|d| > 2j), beyond r = k/2, and at the centre for d != 0."""
    c = torch.arange(k, dtype=torch.float64) - (k - 1) / 2.0
    row, col = torch.meshgrid(c, c, indexing="ij")
    r = torch.sqrt(row * row + col * col)
    phi = torch.atan2(PHI_SIGN * row, col)
    J = k // 2 + 1
    basis = torch.zeros(4 * MAX_FREQ + 1, J, k, k, 2, dtype=torch.float64)
    for j in range(J):
        ring = torch.exp(-(r - j) ** 2 / (2.0 * RING_SIGMA ** 2)) * (r <= k / 2.0)
        for d in range(-2 * MAX_FREQ, 2 * MAX_FREQ + 1):
            if abs(d) > 2 * j:
                continue
            rd = ring if d == 0 else ring * (r > 0)
            basis[d + 2 * MAX_FREQ, j, :, :, 0] = rd * torch.cos(d * phi)
            basis[d + 2 * MAX_FREQ, j, :, :, 1] = rd * torch.sin(d * phi)
    return basis


def _channels(kind: str, m: int) -> Tuple[int, Optional[int]]:
    """(channel of Re, channel of Im or None) of frequency m inside a field of the given kind."""
    if kind == "vector":
        return 0, 1
    return (0, None) if m == 0 else (2 * m - 1, 2 * m)


def _field_dim(kind: str) -> int:
    return {"scalar": 1, "fourier": FIELD_DIM, "vector": 2}[kind]


class _Fp64Tables(nn.Module):
    """Modules whose constant tables are built in fp64 and then cast: a dtype / device change (``.double()``, ``.to(device)``) casts
    them again FROM THE fp64 ORIGINAL, so the fp64 form of the network (the reference of the tests) is not an up-cast fp32 table."""

    def _tables(self) -> Dict[str, torch.Tensor]:
        raise NotImplementedError

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        for name, table in self._tables().items():
            like = getattr(self, name)
            setattr(self, name, table.to(dtype=like.dtype, device=like.device))
        return self


class SteerableConv(_Fp64Tables):
    """k x k steerable convolution between fields of kind "scalar" (frequency 0), "fourier" (0..4) or "vector" (1); stride 1, no
    padding, no bias.

    ``weights``: (out_fields, in_fields, M, N, 2, J, 2) = per (output field, input field, output frequency m, input frequency n,
    term [kappa, kappa'], ring j) one complex weight as (Re, Im).  Slots that carry nothing (kappa' where m = 0 or n = 0, rings
    with |d| > 2j, the imaginary part where m = n = 0) start at zero and receive a zero gradient.
    Initialisation: the non-empty slots (n, term, ring) that feed output frequency m share its variance equally -- slot s draws both
    parts from N(0, 1 / (in_fields * S_m * E_s * c_n)), S_m = number of such slots, E_s = sum_y |R_j e^{id phi}|^2 its basis energy,
    c_n = 2 for a complex input (n > 0: Re and Im both feed every output component), 1 for n = 0 -- so that an input with independent
    unit-variance components gives unit-variance output components (variance kept over the fan-in).
    ``basis``: `steerable_basis(k)`, a buffer.  ``expanded_weights()``: the dense real bank (out_fields * dim_out, in_fields * dim_in,
    k, k), an einsum of weights and basis, differentiable."""

    def __init__(self, in_fields: int, in_kind: str, out_fields: int, out_kind: str, kernel_size: int):
        super().__init__()
        self.in_fields, self.in_kind, self.out_fields, self.out_kind = in_fields, in_kind, out_fields, out_kind
        self.kernel_size, self.stride, self.padding = kernel_size, 1, 0
        self.in_dim, self.out_dim = _field_dim(in_kind), _field_dim(out_kind)
        J = kernel_size // 2 + 1
        M, N = len(_FREQS[out_kind]), len(_FREQS[in_kind])
        self.weights = nn.Parameter(torch.zeros(out_fields, in_fields, M, N, 2, J, 2))
        self._cache = DerivedCache()                             # eval: "bank", the dense bank, and "fft", its spectra: see ESCNNSteerableNetwork
        self.register_buffer("basis", steerable_basis(kernel_size).to(torch.get_default_dtype()))
        for name, table in self._tables().items():
            if name != "basis":
                self.register_buffer(name, table.to(torch.get_default_dtype()), persistent=False)
        self.reset_parameters()

    def _harmonic(self, m: int, n: int, term: int) -> Optional[int]:
        if term == 0:
            return m - n
        return m + n if m > 0 and n > 0 else None

    def _tables(self) -> Dict[str, torch.Tensor]:
        """basis; kernel_parts (M, N, 2, J, 2[w part], 2[kappa part], k, k): kappa = w * basis as a real map of (Re w, Im w);
        blocks (M, N, 2, 2[kappa part], dim_out, dim_in): where kappa's parts go in the real bank -- the block of kappa c_n is
        [[kr, -ki], [ki, kr]], that of kappa' conj(c_n) is [[kr, ki], [ki, -kr]]; m = 0 keeps the Re row, n = 0 the Re column."""
        k = self.kernel_size
        basis = steerable_basis(k)
        mo, ni = _FREQS[self.out_kind], _FREQS[self.in_kind]
        J = k // 2 + 1
        cmul = torch.zeros(2, 2, 2, dtype=torch.float64)          # [w part, basis part, kappa part] of a complex product
        cmul[0, 0, 0], cmul[1, 1, 0], cmul[0, 1, 1], cmul[1, 0, 1] = 1.0, -1.0, 1.0, 1.0
        parts = torch.zeros(len(mo), len(ni), 2, J, 2, 2, k, k, dtype=torch.float64)
        blocks = torch.zeros(len(mo), len(ni), 2, 2, self.out_dim, self.in_dim, dtype=torch.float64)
        for a, m in enumerate(mo):
            for b, n in enumerate(ni):
                o_re, o_im = _channels(self.out_kind, m)
                i_re, i_im = _channels(self.in_kind, n)
                for term in (0, 1):
                    d = self._harmonic(m, n, term)
                    if d is None:
                        continue
                    parts[a, b, term] = torch.einsum("jyxq,pqc->jpcyx", basis[d + 2 * MAX_FREQ], cmul)
                    s = 1.0 if term == 0 else -1.0
                    blocks[a, b, term, 0, o_re, i_re] = 1.0
                    if i_im is not None:
                        blocks[a, b, term, 1, o_re, i_im] = -s
                    if o_im is not None:
                        blocks[a, b, term, 1, o_im, i_re] = 1.0
                    if o_im is not None and i_im is not None:
                        blocks[a, b, term, 0, o_im, i_im] = s
        return {"basis": basis, "kernel_parts": parts, "blocks": blocks}

    def reset_parameters(self) -> None:
        basis = steerable_basis(self.kernel_size)
        energy = (basis ** 2).sum(dim=(2, 3, 4))                 # (17, J)
        mo, ni = _FREQS[self.out_kind], _FREQS[self.in_kind]
        with torch.no_grad():
            self.weights.zero_()
            for a, m in enumerate(mo):
                slots = [(b, term, j, float(energy[d + 2 * MAX_FREQ, j]))
                         for b, n in enumerate(ni) for term in (0, 1)
                         for d in [self._harmonic(m, n, term)] if d is not None
                         for j in range(energy.shape[1]) if float(energy[d + 2 * MAX_FREQ, j]) > 0.0]
                for b, term, j, e in slots:
                    std = 1.0 / math.sqrt(self.in_fields * len(slots) * e * (2 if ni[b] > 0 else 1))
                    parts = 1 if (m == 0 and ni[b] == 0) else 2          # frequency 0 -> 0: only the real part acts
                    self.weights[:, :, a, b, term, j, :parts].normal_(0.0, std)

    def expanded_weights(self) -> torch.Tensor:
        kappa = torch.einsum("oimntjp,mntjpcyx->oimntcyx", self.weights, self.kernel_parts)
        bank = torch.einsum("oimntcyx,mntcab->oaibyx", kappa, self.blocks)
        k = self.kernel_size
        return bank.reshape(self.out_fields * self.out_dim, self.in_fields * self.in_dim, k, k)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.conv2d(x, self.expanded_weights())

    def complex_forward(self, x: torch.Tensor) -> torch.Tensor:
        """The same map written frequency by frequency in complex arithmetic (Re / Im planes, four real convolutions per complex
        one), without the dense bank or its block table: what ``forward`` is tested against."""
        B, _, H, W = x.shape
        k = self.kernel_size
        xs = x.unflatten(1, (self.in_fields, self.in_dim))
        out = x.new_zeros(B, self.out_fields, self.out_dim, H - k + 1, W - k + 1)
        w = torch.view_as_complex(self.weights.contiguous())                        # (O, I, M, N, 2, J)
        basis = torch.view_as_complex(self.basis.contiguous())                      # (17, J, k, k)
        for a, m in enumerate(_FREQS[self.out_kind]):
            o_re, o_im = _channels(self.out_kind, m)
            for b, n in enumerate(_FREQS[self.in_kind]):
                i_re, i_im = _channels(self.in_kind, n)
                re = xs[:, :, i_re]
                im = xs[:, :, i_im] if i_im is not None else torch.zeros_like(re)
                for term in (0, 1):
                    d = self._harmonic(m, n, term)
                    if d is None:
                        continue
                    kappa = torch.einsum("oij,jyx->oiyx", w[:, :, a, b, term], basis[d + 2 * MAX_FREQ])
                    kr, ki = kappa.real.contiguous(), kappa.imag.contiguous()
                    ci = im if term == 0 else -im                                   # kappa' acts on conj(c_n)
                    out[:, :, o_re] += F.conv2d(re, kr) - F.conv2d(ci, ki)
                    if o_im is not None:
                        out[:, :, o_im] += F.conv2d(re, ki) + F.conv2d(ci, kr)
        return out.flatten(1, 2)


def field_norm_scale_shift(sums: torch.Tensor, n: int, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                           dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`FieldNorm`'s batch statistics and affine map from the six sums per field over the n pixels of a map.
    sums:(fields, 6) fp64 = sum a_0, sum a_0^2, sum (Re^2 + Im^2) of c_1..c_4.  Returns mean:(fields,) and var:(fields, 5) in fp64
    (var_0 = max(E[a_0^2] - mean^2, 0), var_m = E[(Re^2 + Im^2) / 2]) and scale:(fields, 5), shift:(fields,) in `dtype`.  All of it
    is fp64 arithmetic on the sums' device, each result rounded to `dtype` once; the shift is formed from the ROUNDED scale,
    so that scale_0 a_0 + shift = scale_0 (a_0 - mean) + bias keeps its accuracy where the mean is large against the spread."""
    sums = sums.double()
    mean = sums[:, 0] / n
    var0 = (sums[:, 1] / n - mean * mean).clamp_min(0.0)
    var = torch.cat([var0[:, None], sums[:, 2:] / (2.0 * n)], dim=1)
    scale = (weight.double() * torch.rsqrt(var + eps)).to(dtype)
    shift = (bias.double() - mean * scale[:, 0].double()).to(dtype)
    return mean, var, scale, shift


def field_norm_backward_coefficients(bsums: torch.Tensor, weight: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, n: int,
                                     eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The backward of `FieldNorm` (training mode) through its batch statistics, from six sums per field.
    bsums:(fields, 6) fp64 = S_0 = sum du_0, S_1 = sum du_0 a_0, T_m = sum (du_Re Re + du_Im Im) of c_m, du the gradient at the norm's
    output; mean, var: the batch statistics of `field_norm_scale_shift`.  With r = rsqrt(var + eps), scale = weight r and
    D = r_0 (S_1 - mean S_0):  dbias = S_0,  dweight = (D, r_m T_m),  and the gradient at the norm's input is
      dx_0 = scale_0 du_0 - k_0 - c_1 (a_0 - mean),  dx_j = scale_m du_j - c_{1+m} x_j  (both parts of frequency m),
      k_0 = scale_0 S_0 / n,  c_1 = scale_0 r_0 D / n,  c_{1+m} = scale_m r_m^2 T_m / (2 n)
    (the clamp of var_0 at zero passes its gradient, as `clamp_min` does at and above 0).
    Returns coef:(fields, 7) = (k_0, mean, c_1..c_5), dweight:(fields, 5), dbias:(fields,), all fp64."""
    bsums, mean, var = bsums.double(), mean.double(), var.double()
    r = torch.rsqrt(var + eps)
    scale = weight.double() * r
    S0, S1, T = bsums[:, 0], bsums[:, 1], bsums[:, 2:]
    D = r[:, 0] * (S1 - mean * S0)
    dweight = torch.cat([D[:, None], r[:, 1:] * T], dim=1)
    k0 = scale[:, 0] * S0 / n
    c1 = scale[:, 0] * r[:, 0] * D / n
    cm = scale[:, 1:] * r[:, 1:] ** 2 * T / (2.0 * n)
    return torch.cat([k0[:, None], mean[:, None], c1[:, None], cm], dim=1), dweight, S0


class FieldNormFourierELUFunction(torch.autograd.Function):
    """FourierELU(FieldNorm(x)) with batch statistics on a channels-last fp32 device map: statistics (csrc/field_norm.hip), their
    finalisation in fp64 torch ops on the device (no host synchronisation), `ops.fourier_elu` with the resulting scale / shift.
    Returns (y, mean:(fields,), var:(fields, 5)), the statistics not differentiable (the running averages want them).  Saves x and
    per-field tables only -- never the normed map: the backward is one reduction over (x, dy), the same finalisation, and one pass
    that forms the activation's gradient again and writes dx.
    sums: the (fields, 6) fp64 sums of x where the kernel that wrote x took them on the way out (`SteerLiftFunction`); then
    `ops.field_norm_stats` is not launched."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, sums=None):
        x = x.contiguous(memory_format=torch.channels_last)
        n = x.shape[0] * x.shape[2] * x.shape[3]
        if sums is None:
            sums = ops.field_norm_stats(x).sum(0)
        mean, var, scale, shift = field_norm_scale_shift(sums, n, weight.detach(), bias.detach(), eps)
        ctx.save_for_backward(x, weight, scale, shift, mean, var)
        ctx.eps, ctx.n = eps, n
        mean32, var32 = mean.float(), var.float()
        ctx.mark_non_differentiable(mean32, var32)
        return ops.fourier_elu(x, scale, shift), mean32, var32

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _dmean, _dvar):
        x, weight, scale, shift, mean, var = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        bsums = ops.field_norm_elu_bwd_reduce(x, dy, scale, shift).sum(0)
        coef, dweight, dbias = field_norm_backward_coefficients(bsums, weight, mean, var, ctx.n, ctx.eps)
        dx = ops.field_norm_elu_bwd_apply(x, dy, scale, shift, coef.float()) if ctx.needs_input_grad[0] else None
        return dx, dweight.to(weight.dtype), dbias.to(weight.dtype), None, None


class FieldNorm(nn.Module):
    """This package's norm for "fourier" fields, in the place of e2cnn's ``GNormBatchNorm`` (whose arithmetic cannot be checked
    here): frequency 0 is ordinary batch norm over (B, H, W) with weight and bias; frequency m >= 1 is
    c_m * weight / sqrt(E[(Re^2 + Im^2) / 2] + eps) -- no mean subtracted, no bias, so it commutes with the rotation of the field.
    eps = 1e-5, momentum 0.1; running statistics are buffers (``running_var[:, 0]`` the unbiased variance of a_0 as in
    nn.BatchNorm2d, ``running_var[:, m]`` the mean square of frequency m)."""

    def __init__(self, fields: int, eps: float = 1e-5, momentum: float = 0.1):
        super().__init__()
        self.fields, self.eps, self.momentum = fields, eps, momentum
        self.weight = nn.Parameter(torch.ones(fields, MAX_FREQ + 1))
        self.bias = nn.Parameter(torch.zeros(fields))
        self.register_buffer("running_mean", torch.zeros(fields))
        self.register_buffer("running_var", torch.ones(fields, MAX_FREQ + 1))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self._cache = DerivedCache()

    def _scale_shift(self, mean: torch.Tensor, var: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        scale = self.weight * torch.rsqrt(var + self.eps)                     # (fields, 5)
        return scale, self.bias - mean * scale[:, 0]

    def folded(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scale (fields, 5), shift (fields,)) of the eval-mode norm, what `ops.fourier_elu` applies on its loads."""
        def build():
            with torch.no_grad():
                scale, shift = self._scale_shift(self.running_mean, self.running_var)
            return scale.contiguous(), shift.contiguous()

        return self._cache.get("folded", (self.weight, self.bias, self.running_mean, self.running_var), build)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        C = self.fields
        if self.training:
            xs = x.unflatten(1, (C, FIELD_DIM))
            a0 = xs[:, :, 0]
            n = a0.numel() // C
            mean = a0.mean(dim=(0, 2, 3))
            var0 = (a0 * a0).mean(dim=(0, 2, 3)) - mean * mean
            var0 = var0.clamp_min(0.0)
            ms = (xs[:, :, 1:] ** 2).unflatten(2, (MAX_FREQ, 2)).mean(dim=(0, 3, 4, 5))      # (fields, 4): E[(Re^2 + Im^2) / 2]
            var = torch.cat([var0[:, None], ms], dim=1)
            with torch.no_grad():
                unbiased = torch.cat([var0[:, None] * (n / max(n - 1, 1)), ms], dim=1)
                self.running_mean.mul_(1.0 - self.momentum).add_(mean.to(self.running_mean.dtype), alpha=self.momentum)
                self.running_var.mul_(1.0 - self.momentum).add_(unbiased.to(self.running_var.dtype), alpha=self.momentum)
                self.num_batches_tracked += 1
        else:
            mean, var = self.running_mean, self.running_var
        scale, shift = self._scale_shift(mean, var)
        idx = [0] + [(j + 1) // 2 for j in range(1, FIELD_DIM)]
        scale9 = scale[:, idx].reshape(1, C * FIELD_DIM, 1, 1)
        shift9 = F.pad(shift[:, None], (0, FIELD_DIM - 1)).reshape(1, C * FIELD_DIM, 1, 1)
        return x * scale9 + shift9

    def forward_elu(self, x: torch.Tensor, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
        """FourierELU(self(x)) in training mode on a channels-last fp32 device map, on the kernels (`FieldNormFourierELUFunction`),
        with the running-statistics update of `forward`.  sums: x's (fields, 6) sums, where its producer took them."""
        y, mean, var = FieldNormFourierELUFunction.apply(x, self.weight, self.bias, self.eps, sums)
        n = x.shape[0] * x.shape[2] * x.shape[3]
        with torch.no_grad():
            unbiased = torch.cat([var[:, :1] * (n / max(n - 1, 1)), var[:, 1:]], dim=1)
            self.running_mean.mul_(1.0 - self.momentum).add_(mean.to(self.running_mean.dtype), alpha=self.momentum)
            self.running_var.mul_(1.0 - self.momentum).add_(unbiased.to(self.running_var.dtype), alpha=self.momentum)
            self.num_batches_tracked += 1
        return y


def fused_field_norm(norm: FieldNorm) -> bool:
    """Whether a hidden block of the device path runs `norm.forward_elu`: the norm takes batch statistics, neither kernel knob is
    off, and the field-norm kernels take its field count."""
    return (norm.training and os.environ.get(_FOURIER_ACT_KERNEL, "1") != "0" and os.environ.get(_FIELD_NORM_KERNEL, "1") != "0"
            and norm.fields <= ops.FIELD_NORM_MAX_FIELDS)


class SteerLiftFunction(torch.autograd.Function):
    """The scalar -> Fourier-field convolution of the first layer on the kernels of csrc/steer_lift.hip: y = conv2d(x, bank) on a
    channels-last fp32 device map (`ops.steer_lift`), filter gradient on the matrix cores too (`ops.steer_lift_wgrad`).  The input
    image needs no gradient in the canonicalizer; if asked for, it is the framework's.  with_stats: also return the (fields, 6)
    fp64 sums the field norm behind the layer needs, taken in the kernel's epilogue (not differentiable)."""

    @staticmethod
    def forward(ctx, x, bank, with_stats=False):
        ctx.save_for_backward(x, bank)
        k, fields = bank.shape[-1], bank.shape[0] // FIELD_DIM
        y, sums = ops.steer_lift(x, ops.pack_steer_lift_weights(bank.detach()), k, fields, with_stats)
        if with_stats:
            ctx.mark_non_differentiable(sums)
            return y, sums
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, *_):
        x, bank = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.nn.grad.conv2d_input(x.shape, bank, dy) if ctx.needs_input_grad[0] else None
        dbank = ops.steer_lift_wgrad(x, dy, bank.shape[-1]) if ctx.needs_input_grad[1] else None
        return dx, dbank, None


def steer_lift_route(conv: "SteerableConv", h: torch.Tensor) -> bool:
    """Whether `conv` on the channels-last fp32 device map h runs on the steerable lifting kernels: a scalar -> Fourier-field layer of a
    shape they take, a map of at least k x k, and the knob not off.
    Measured exclusions (tools/kbench_steer_lift.py, profiles/steer_lift/): see DESIGN.md, ESCNNSteerableNetwork / Speed."""
    k = conv.kernel_size
    return (conv.in_kind == "scalar" and conv.out_kind == "fourier" and os.environ.get(_STEER_LIFT_KERNEL, "1") != "0"
            and h.shape[0] > 0 and h.shape[2] >= k and h.shape[3] >= k and ops.steer_lift_supported(conv.in_fields, k, conv.out_fields))


class FourierELUFunction(torch.autograd.Function):
    """y = A^+ ELU(A x) on a channels-last fp32 device map, forward and backward on the kernels of csrc/fourier_act.hip.  Saves x
    only: the backward recomputes the 16 samples."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x)
        return ops.fourier_elu(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.fourier_elu_bwd(x, dy.contiguous(memory_format=torch.channels_last))


class FourierELU(_Fp64Tables):
    """ELU applied to the 16 samples of every field, projected back onto frequencies 0..4: y = (A^T / 16) ELU(A x) per pixel and
    field (e2cnn's FourierELU with N = 16).  Commutes with the rotations by multiples of 2 pi / 16 exactly; for other angles the
    projection drops what ELU puts above frequency 4.  This module is the plain-op form (CPU, fp64; the reference of the kernel)."""

    def __init__(self, fields: int):
        super().__init__()
        self.fields = fields
        self.register_buffer("A", sampling_matrix().to(torch.get_default_dtype()), persistent=False)

    def _tables(self) -> Dict[str, torch.Tensor]:
        return {"A": sampling_matrix()}

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        xs = x.unflatten(1, (self.fields, FIELD_DIM))
        s = F.elu(torch.einsum("ij,bcjhw->bcihw", self.A, xs))
        return torch.einsum("ij,bcihw->bcjhw", self.A / NUM_SAMPLES, s).flatten(1, 2)


class ESCNNSteerableNetwork(nn.Module):
    """See the module docstring.  ``forward``: (B, Cin, H, W) -> (B, 2, 2).

    CPU tensors and fp64 run through plain torch ops (``self.block``, then the spatial mean).  fp32 device tensors run the same
    layers channels-last with the activation on the HIP kernels: in eval mode without autograd the norm's running statistics fold
    into the kernel's scale / shift (norm + activation: one pass over the map) and the dense banks are cached per weight version;
    a norm in training mode is `FieldNorm.forward_elu` (batch statistics, norm + activation and their backward on the kernels of
    csrc/field_norm.hip and csrc/fourier_act.hip); otherwise (a frozen norm inside a training step, more fields than those kernels
    take, `EQA_FIELD_NORM_KERNEL=0`) the norm stays in torch ops and the activation is `FourierELUFunction`.  A hidden -> hidden convolution whose shape
    `fftconv.applicable_k` admits is the overlap-save FFT convolution (`fftconv.conv_kxk` / `fftconv.ConvKxKFunction`), every other
    one the library's on channels-last.  The first layer (scalar -> Fourier fields) is the fused lifting kernel of
    csrc/steer_lift.hip where `steer_lift_route` admits it (`SteerLiftFunction` in training, which also hands the norm behind it
    its batch sums); `EQA_STEER_LIFT_KERNEL=0` keeps the library's convolution.  ``last_routes``: one word per convolution of the
    last device forward ("steer_lift", "fft", "lib", "window_sums").  The tail (last convolution + spatial mean) is linear, so where the window-sum kernels take
    the shape it is window sums times the tail bank."""

    def __init__(self, in_shape: tuple, out_channels: int, kernel_size: int = 9, group_type: str = "rotation", num_layers: int = 1):
        super().__init__()
        self.group_type = group_type
        assert group_type == "rotation", "group_type must be rotation for now."
        self.in_channels, self.out_channels, self.kernel_size, self.num_layers = in_shape[0], out_channels, kernel_size, num_layers
        mods: List[nn.Module] = []
        fields, kind = self.in_channels, "scalar"
        for _ in range(num_layers):
            mods += [SteerableConv(fields, kind, out_channels, "fourier", kernel_size), FieldNorm(out_channels), FourierELU(out_channels)]
            fields, kind = out_channels, "fourier"
        mods.append(SteerableConv(fields, kind, 2, "vector", kernel_size))
        self.block = nn.Sequential(*mods)
        self.last_routes: List[str] = []

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """A checkpoint of the reference's e2cnn network cannot be loaded by key: e2cnn stores one flat coefficient vector per
        R2Conv over its own steerable basis (``...weights`` 1-D, ``...basisexpansion...`` / ``...filter`` buffers) and GNormBatchNorm
        statistics per irrep (``..._running_var`` / ``..._weight`` named after the irrep); this network's weights are complex
        ring / harmonic coefficients.  Say so instead of failing on a missing key or a shape mismatch."""
        refuse_e2cnn_state_dict(
            state_dict, prefix + "block.", "ESCNNSteerableNetwork",
            "equiadapt_amd.ESCNNSteerableNetwork keeps the reference's constructor, layer order and output contract but "
            "parameterises its convolutions by complex ring / harmonic weights of its own and uses its own field norm: it is "
            "a different function class, e2cnn checkpoints cannot be loaded, and there is no bridge for them.", ("irrep_",))
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @staticmethod
    def _bank(conv: SteerableConv, cache: bool) -> torch.Tensor:
        """conv's dense bank, channels-last; in eval without autograd kept on the layer."""
        if not cache:
            return conv.expanded_weights().contiguous(memory_format=torch.channels_last)
        return conv._cache.get("bank", (conv.weights, conv.kernel_parts, conv.blocks),
                               lambda: conv.expanded_weights().detach().contiguous(memory_format=torch.channels_last))

    def _conv(self, h: torch.Tensor, conv: SteerableConv, infer: bool, want_sums: bool = False):
        """conv on the channels-last device map h -> (map, sums, route): the fused lifting kernel for the first layer, the FFT
        convolution where its own gate admits the dense bank, else the library's.  sums: the (fields, 6) sums for the field norm
        behind the layer where want_sums and the route takes them on the way out, else None."""
        k = conv.kernel_size
        cout, cin = conv.out_fields * conv.out_dim, conv.in_fields * conv.in_dim
        if steer_lift_route(conv, h):
            if not infer:
                out = SteerLiftFunction.apply(h, conv.expanded_weights(), want_sums)
                return (*out, "steer_lift") if want_sums else (out, None, "steer_lift")
            bank = self._bank(conv, True)
            wpk = conv._cache.derived("bank", "steer_lift", lambda: ops.pack_steer_lift_weights(bank))
            return ops.steer_lift(h, wpk, k, conv.out_fields)[0], None, "steer_lift"
        if conv.in_kind == "fourier" and fftconv.applicable_k(h.shape, cin, cout, k, h.device,
                                                              h.is_contiguous(memory_format=torch.channels_last)):
            if not infer:
                return fftconv.ConvKxKFunction.apply(h, conv.expanded_weights()), None, "fft"
            bank = self._bank(conv, True)
            return fftconv.conv_kxk(h, conv._cache.derived("bank", "fft", lambda: fftconv.spectra_for_k(bank)), k, None, False), None, "fft"
        return F.conv2d(h, self._bank(conv, infer)), None, "lib"

    @staticmethod
    def _tail(h: torch.Tensor, conv: SteerableConv, bank: torch.Tensor, infer: bool) -> Tuple[torch.Tensor, str]:
        """(spatial mean of the last convolution, (B, 4); its route).  Where the channels-last window-sum kernel takes the map: its k x k window
        sums (fp64) times the bank; else the convolution and a mean."""
        k = conv.kernel_size
        B, C, H, W = h.shape
        if (C % 4 == 0 and k <= ops.MAX_WINDOW_K and H > 2 * (k - 1) and W > 2 * (k - 1) and 0 < B <= 65535
                and not h.is_contiguous() and h.is_contiguous(memory_format=torch.channels_last)):
            S = ops.window_sums(h, k) if infer else WindowSumsFunction.apply(h, k)           # (B, C, k, k) fp64
            return (S.flatten(1) @ bank.double().flatten(1).t() / float((H - k + 1) * (W - k + 1))).float(), "window_sums"
        return F.conv2d(h, bank).mean(dim=(-2, -1)), "lib"

    def _forward_device(self, x: torch.Tensor) -> torch.Tensor:
        infer = not self.training and not torch.is_grad_enabled()
        kernel = os.environ.get(_FOURIER_ACT_KERNEL, "1") != "0"
        mods = list(self.block)
        h = x.contiguous(memory_format=torch.channels_last)
        routes: List[str] = []
        for i in range(0, len(mods) - 1, 3):
            conv, norm, act = mods[i:i + 3]
            fused = kernel and fused_field_norm(norm)
            h, sums, route = self._conv(h, conv, infer, want_sums=fused)
            routes.append(route)
            if not kernel:
                h = act(norm(h)).contiguous(memory_format=torch.channels_last)
            elif fused:
                h = norm.forward_elu(h, sums)
            elif infer and not norm.training:
                h = ops.fourier_elu(h.contiguous(memory_format=torch.channels_last), *norm.folded())
            else:
                h = FourierELUFunction.apply(norm(h))
        out, route = self._tail(h, mods[-1], self._bank(mods[-1], infer), infer)
        self.last_routes = routes + [route]
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and x.dtype == torch.float32:
            out = self._forward_device(x)
        else:
            out = self.block(x).mean(dim=(-2, -1))
        return out.reshape(x.shape[0], 2, 2)
