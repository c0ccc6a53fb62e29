"""Vector-neuron layers (reference: pointcloud/canonicalization_networks/vector_neuron_layers.py).

The layers of VNSmall's hot path (VNLinearLeakyReLU :210-273, VNBatchNorm :276-324, VNMaxPool :327-364, mean_pool :367-380) and the
rest of the reference file (VNLinear :16-49, VNBilinear :52-90, VNSoftplus :93-151, VNLeakyReLU :154-207, VNStdFeature :383-492);
module and parameter names match the reference state_dict.
Features are [B, C, 3, N, ...]: every channel is a 3-vector, linear maps mix channels only, so all layers
commute with rotations of the 3-axis.

VNLeakyReLU and VNSoftplus have two routes: the reference's op sequence ("plain": any device, any dtype, full autograd) and, for
fp32 tensors on the device with at most `ops.vn_act_max_channels()` channels, one fused kernel each way (csrc/vn_act.hip: one read
of x, one write of y).  ``EQA_VN_ACT_KERNEL=0`` forces the plain route.  ``last_route`` records which one the last call took.
"""
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

EPS = 1e-6


def _mix_channels(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """Apply a bias-free linear map over the channel axis (dim 1) of [B, C, 3, ...]."""
    W = lin.weight                                                   # (out, in)
    if x.is_cuda and W.shape[1] <= 4 and torch.is_grad_enabled():
        # conv_pos: 3 input channels on a (B, 3, 3, N, k) edge tensor.  As a GEMM this is 3.9 M rows x K = 3 (measured 5.8 ms
        # per map in the library at B = 64); as `in` fused multiply-adds over the output it is three streaming passes.
        # Training only: without autograd the GEMM form is kept, whose rounding the max-pooling golden vectors are pinned to
        # (an argmax over near-ties flips on a last-bit difference)
        shape = [1, W.shape[0]] + [1] * (x.dim() - 2)
        out = W[:, 0].view(shape) * x[:, 0:1]
        for i in range(1, W.shape[1]):
            out = torch.addcmul(out, W[:, i].view(shape), x[:, i:i + 1])
        return out
    return lin(x.transpose(1, -1)).transpose(1, -1)


class VNBatchNorm(nn.Module):
    """x / |x| * BN(|x| + EPS): batch-normalises the vector norms, keeps directions."""

    def __init__(self, num_features: int, dim: int):
        super().__init__()
        self.dim = dim
        if dim in (3, 4):
            self.bn1d = nn.BatchNorm1d(num_features)
        elif dim == 5:
            self.bn2d = nn.BatchNorm2d(num_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        norm = torch.norm(x, dim=2) + EPS
        norm_bn = self.bn2d(norm) if self.dim == 5 else self.bn1d(norm)
        return x / norm.unsqueeze(2) * norm_bn.unsqueeze(2)


class VNLinearLeakyReLU(nn.Module):
    """q = VNBN(W_f x); d = W_d x; keep q where <q,d> >= 0, else remove its component along d."""

    def __init__(self, in_channels: int, out_channels: int, dim: int = 5, share_nonlinearity: bool = False,
                 negative_slope: float = 0.2):
        super().__init__()
        self.dim = dim
        self.negative_slope = negative_slope
        self.map_to_feat = nn.Linear(in_channels, out_channels, bias=False)
        self.batchnorm = VNBatchNorm(out_channels, dim=dim)
        self.map_to_dir = nn.Linear(in_channels, 1 if share_nonlinearity else out_channels, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        q = self.batchnorm(_mix_channels(self.map_to_feat, x))
        d = _mix_channels(self.map_to_dir, x)
        dot = (q * d).sum(2, keepdim=True)
        keep = (dot >= 0).float()
        dsq = (d * d).sum(2, keepdim=True)
        s = self.negative_slope
        return s * q + (1 - s) * (keep * q + (1 - keep) * (q - (dot / (dsq + EPS)) * d))


class VNMaxPool(nn.Module):
    """Along the last axis pick the sample with the largest <x, W_d x> (per batch, channel, point)."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.map_to_dir = nn.Linear(in_channels, in_channels, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        d = _mix_channels(self.map_to_dir, x)
        idx = (x * d).sum(2, keepdim=True).max(dim=-1, keepdim=True)[1]
        return torch.gather(x, -1, idx.expand(*x.shape[:-1], 1)).squeeze(-1)


def mean_pool(x: torch.Tensor, dim: int = -1, keepdim: bool = False) -> torch.Tensor:
    return x.mean(dim=dim, keepdim=keepdim)


_VN_ACT_KERNEL = "EQA_VN_ACT_KERNEL"     # "0": the plain route on the device as well (A/B timing: tools/kbench_vn_act.py)


class _VNActFunction(torch.autograd.Function):
    """The fused directional nonlinearity (ops.vn_act / ops.vn_act_backward); only x and Wd are saved."""

    @staticmethod
    def forward(ctx, x, Wd, softplus, slope):
        from equiadapt_amd import ops

        x = x.contiguous()
        ctx.save_for_backward(x, Wd)
        ctx.softplus, ctx.slope = softplus, slope
        return ops.vn_act(x, Wd, softplus, slope)

    @staticmethod
    def backward(ctx, gy):
        from equiadapt_amd import ops

        x, Wd = ctx.saved_tensors
        gx, gW = ops.vn_act_backward(x, Wd, gy, ctx.softplus, ctx.slope)
        return gx, gW, None, None


def _vn_act_route(x: torch.Tensor, W: torch.Tensor) -> str:
    """Either "fused" or "plain: <why>", for the directional nonlinearity of x with the direction map W."""
    if os.environ.get(_VN_ACT_KERNEL, "1") == "0":
        return f"plain: {_VN_ACT_KERNEL}=0"
    if not (x.is_cuda and W.is_cuda):
        return "plain: not on the device"
    if x.dtype != torch.float32 or W.dtype != torch.float32:
        return f"plain: {x.dtype}, the kernel is fp32"
    if x.dim() < 3 or x.shape[2] != 3 or x.numel() == 0:
        return "plain: not a non-empty (B, C, 3, ...) tensor"
    from equiadapt_amd import ops

    limit = ops.vn_act_max_channels()
    if x.shape[1] > limit:
        return f"plain: {x.shape[1]} channels, the kernel takes {limit}"
    return "fused"


def _directional_act(module: nn.Module, x: torch.Tensor, softplus: bool) -> torch.Tensor:
    """slope x + (1 - slope) (mask x + (1 - mask) (x - (<x,d> / (|d|^2 + EPS)) d)),  d = W_d x."""
    s = module.negative_slope
    module.last_route = _vn_act_route(x, module.map_to_dir.weight)
    if module.last_route == "fused":
        return _VNActFunction.apply(x, module.map_to_dir.weight, softplus, float(s))
    d = _mix_channels(module.map_to_dir, x)
    dot = (x * d).sum(2, keepdim=True)
    if softplus:
        angle = torch.acos(dot / (torch.norm(x, dim=2, keepdim=True) * torch.norm(d, dim=2, keepdim=True) + EPS))
        mask = torch.cos(angle / 2) ** 2
    else:
        mask = (dot >= 0).to(x.dtype)
    dsq = (d * d).sum(2, keepdim=True)
    return s * x + (1 - s) * (mask * x + (1 - mask) * (x - (dot / (dsq + EPS)) * d))


class VNLinear(nn.Module):
    """W_f x over the channel axis, no bias."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.map_to_feat = nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _mix_channels(self.map_to_feat, x)


class VNBilinear(nn.Module):
    """Bias-free bilinear map of the channels of x:[B, C1, 3] with labels:[B, 1, C2] (repeated over the 3-axis).

    As in the reference, only a 3-D x works: a 4-D or 5-D x raises inside nn.functional.bilinear (the repeated labels no longer
    match x's leading axes).  That behaviour is kept, not repaired."""

    def __init__(self, in_channels1: int, in_channels2: int, out_channels: int):
        super().__init__()
        self.map_to_feat = nn.Bilinear(in_channels1, in_channels2, out_channels, bias=False)

    def forward(self, x: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        labels = labels.repeat(1, x.shape[2], 1).float()
        return self.map_to_feat(x.transpose(1, -1), labels).transpose(1, -1)


class VNSoftplus(nn.Module):
    """d = W_d x; x minus a share (1 - slope) (1 - mask) of its component along d, mask = cos^2(angle(x, d) / 2).

    The fused route evaluates the mask as (1 + c) / 2, c = <x,d> / (|x||d| + EPS): the same value without acos, and a finite gradient
    where d is parallel to x (always so for in_channels = 1), where the plain route's gradient through acos, like the reference's,
    is not finite."""

    def __init__(self, in_channels: int, share_nonlinearity: bool = False, negative_slope: float = 0.0):
        super().__init__()
        self.map_to_dir = nn.Linear(in_channels, 1 if share_nonlinearity else in_channels, bias=False)
        self.negative_slope = negative_slope
        self.last_route: Optional[str] = None      # "fused" | "plain: <why>"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _directional_act(self, x, softplus=True)


class VNLeakyReLU(nn.Module):
    """d = W_d x; keep x where <x,d> >= 0, else remove a share (1 - slope) of its component along d."""

    def __init__(self, in_channels: int, share_nonlinearity: bool = False, negative_slope: float = 0.2):
        super().__init__()
        self.map_to_dir = nn.Linear(in_channels, 1 if share_nonlinearity else in_channels, bias=False)
        self.negative_slope = negative_slope
        self.last_route: Optional[str] = None      # "fused" | "plain: <why>"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _directional_act(self, x, softplus=False)


class VNStdFeature(nn.Module):
    """Invariant features: z0 = W (vn2(vn1(x))) gives 3 vectors per point (2, completed to an orthonormal frame, with
    normalize_frame); x_std = x contracted with z0 over the 3-axis.  Returns (x_std, z0).

    The third frame vector is torch.linalg.cross(u1, u2, dim=1).  The reference's torch.cross without `dim` takes the first axis of
    size 3, which is the batch axis when B == 3; for every other B the two agree."""

    def __init__(self, in_channels: int, dim: int = 4, normalize_frame: bool = False, share_nonlinearity: bool = False,
                 negative_slope: float = 0.2):
        super().__init__()
        self.dim = dim
        self.normalize_frame = normalize_frame
        self.vn1 = VNLinearLeakyReLU(in_channels, in_channels // 2, dim=dim, share_nonlinearity=share_nonlinearity,
                                     negative_slope=negative_slope)
        self.vn2 = VNLinearLeakyReLU(in_channels // 2, in_channels // 4, dim=dim, share_nonlinearity=share_nonlinearity,
                                     negative_slope=negative_slope)
        self.vn_lin = nn.Linear(in_channels // 4, 2 if normalize_frame else 3, bias=False)

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        z0 = _mix_channels(self.vn_lin, self.vn2(self.vn1(x)))
        if self.normalize_frame:
            v1 = z0[:, 0, :]
            u1 = v1 / (torch.sqrt((v1 * v1).sum(1, keepdim=True)) + EPS)
            v2 = z0[:, 1, :]
            v2 = v2 - (v2 * u1).sum(1, keepdim=True) * u1
            u2 = v2 / (torch.sqrt((v2 * v2).sum(1, keepdim=True)) + EPS)
            u3 = torch.linalg.cross(u1, u2, dim=1)
            z0 = torch.stack([u1, u2, u3], dim=1).transpose(1, 2)
        else:
            z0 = z0.transpose(1, 2)
        if self.dim == 4:
            x_std = torch.einsum("bijm,bjkm->bikm", x, z0)
        elif self.dim == 3:
            x_std = torch.einsum("bij,bjk->bik", x, z0)
        elif self.dim == 5:
            x_std = torch.einsum("bijmn,bjkmn->bikmn", x, z0)
        return x_std, z0
