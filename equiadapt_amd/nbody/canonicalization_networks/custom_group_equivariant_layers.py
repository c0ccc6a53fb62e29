"""Vector-neuron nonlinearities of the n-body canonicalization network.

Reference: equiadapt/nbody/canonicalization_networks/custom_group_equivariant_layers.py:1-99.  Input ``(M, C, 3)``: ``C`` vector
channels, the spatial axis last.  ``map_to_dir`` mixes channels, the nonlinearity acts on each channel's 3-vector.
"""
import torch
import torch.nn as nn

EPS = 1e-6


class _VNDirectional(nn.Module):
    def __init__(self, in_channels: int, share_nonlinearity: bool, negative_slope: float) -> None:
        super().__init__()
        self.map_to_dir = nn.Linear(in_channels, 1 if share_nonlinearity else in_channels, bias=False)
        self.negative_slope = negative_slope

    def _mask(self, x: torch.Tensor, d: torch.Tensor, dotprod: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        d = self.map_to_dir(x.transpose(1, -1)).transpose(1, -1)
        dotprod = (x * d).sum(2, keepdim=True)
        mask = self._mask(x, d, dotprod)
        d_norm_sq = (d * d).sum(2, keepdim=True)
        return self.negative_slope * x + (1 - self.negative_slope) * (
            mask * x + (1 - mask) * (x - (dotprod / (d_norm_sq + EPS)) * d))


class VNSoftplus(_VNDirectional):
    """mask = cos^2(angle(x, d) / 2): a smooth blend between keeping x and projecting d out of it."""

    def __init__(self, in_channels: int, share_nonlinearity: bool = False, negative_slope: float = 0.0) -> None:
        super().__init__(in_channels, share_nonlinearity, negative_slope)

    def _mask(self, x, d, dotprod):
        angle_between = torch.acos(dotprod / (torch.norm(x, dim=2, keepdim=True) * torch.norm(d, dim=2, keepdim=True) + EPS))
        return torch.cos(angle_between / 2) ** 2


class VNLeakyReLU(_VNDirectional):
    """mask = [<x, d> >= 0]: x is kept where it points along d, d is projected out of it elsewhere."""

    def __init__(self, in_channels: int, share_nonlinearity: bool = False, negative_slope: float = 0.2) -> None:
        super().__init__(in_channels, share_nonlinearity, negative_slope)

    def _mask(self, x, d, dotprod):
        return (dotprod >= 0).to(x.dtype)
