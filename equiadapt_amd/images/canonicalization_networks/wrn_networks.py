"""ESCNNWRNEquivariantNetwork, ESCNNWideBottleneck, ESCNNWideBasic: the wide-ResNet G-CNN canonicalization network.

Reference: equiadapt/images/canonicalization_networks/escnn_networks.py:228-511, built there from e2cnn ``R2Conv`` +
``InnerBatchNorm(momentum=0.9)`` + ``ReLU`` over regular fields; it is the network of the reference's segmentation recipe
(``canonicalization.network_type=equivariant_wrn``).

As with ESCNNEquivariantNetwork, e2cnn's steerable basis is not restated: every convolution is one of this package's rotated-filter-bank
layers (custom_group_equivariant_layers; with quarter turns as exact permutations of the filter taps: `_ExactQuarterTurns`), every
InnerBatchNorm a BatchNorm3d over (B, fields, |G|, H, W).  Constructor, layer order,
field counts, kernel sizes, paddings and the output contract ((B, |G|) = mean over fields and space) are the reference's; the two
block classes take field counts and the group instead of e2cnn ``FieldType``s.  A reference checkpoint does not load by key.

Three routes (``net.last_routes``: one string per convolution, in module order -- a bottleneck's 1 x 1, k x k, 1 x 1; a basic block's
two k x k and its shortcut -- naming what ran):
  plain   F.conv2d on the expanded banks, the batch-norm modules, ReLU, adds: any dtype and device the banks exist on, autograd,
          training mode.  What neither of the other two takes runs here, and so does everything under EQA_WRN_KERNEL=0.
  train   training mode or gradients enabled, fp32 on the device, channel counts on the multiples of 4, and at least one bottleneck
          1 x 1 layer that the kernels take (`_train_ok`): channels-last throughout with autograd (`_forward_training`) -- the 1 x 1
          layers on `GConv1x1Function` (eqa_gconv1x1_nhwc forward and data gradient, eqa_gconv1x1_wgrad filter and bias gradient;
          the second one with the block input as the residual), the k x k layers on the Winograd / FFT convolution Functions, the
          stem on LiftConvFunction, every InnerBatchNorm + ReLU on the fused batch-norm kernels, the tail as window sums; a layer
          whose shape a kernel does not take runs on the library's convolution.  A network without an admitted bottleneck 1 x 1
          layer (num_layers = 3; narrow ones) stays on the plain route.
  fused   eval mode, no_grad, fp32 on the device: channels-last throughout, the batch-norms behind a convolution folded into its
          bank; the two 1 x 1 convolutions of a bottleneck on eqa_gconv1x1_nhwc (csrc/gconv1x1.hip) -- the second with the residual
          add, the InnerBatchNorm behind the block and the ReLU in its epilogue: the junction is one launch --, the k x k layers on the
          FFT / Winograd convolutions where their rules admit the (zero-padded) map, else the library's convolution; the lifting stem
          on the fp32-MFMA lifting kernels; the last convolution and the mean as window sums.  A layer whose shape a kernel does not
          take runs on the library's convolution and torch ops; the rest of the network stays fused.
"""
import os
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from equiadapt_amd import ops
from equiadapt_amd.common.derived import DerivedCache, bn_eval_affine, refuse_e2cnn_state_dict
from equiadapt_amd.images.canonicalization_networks import fftconv, winograd
from equiadapt_amd.images.canonicalization_networks.custom_group_equivariant_layers import (
    RotationEquivariantConv,
    RotationEquivariantConvLift,
    RotoReflectionEquivariantConv,
    RotoReflectionEquivariantConvLift,
    filter_action_matrices,
)
from equiadapt_amd.images.canonicalization_networks.escnn_networks import (
    ESCNNEquivariantNetwork,
    InnerBnReluDropout,
    LiftConvFunction,
    _InnerBatchNorm,
)
from equiadapt_amd.images.canonicalization_networks.pooling import (
    WindowSumsFunction,
    WindowSumsLinearFn,
    conv_then_group_pool,
    group_pool,
)


class GConv1x1Function(torch.autograd.Function):
    """y = conv1x1(x) + bias [+ res] on a channels-last map through eqa_gconv1x1_nhwc (the residual in its epilogue; no affine map, no
    ReLU), with its gradients: dx = conv1x1(dy) with the transposed bank -- the same kernel on the packed transpose, zero bias --,
    dbank and dbias from eqa_gconv1x1_wgrad, dres = dy.  Each only where it is needed.  bank: (Cout, Cin, 1, 1); bias: (Cout,).
    The caller has asked `ops.gconv1x1_supported` and `ops.gconv1x1_wgrad_supported`."""

    @staticmethod
    def forward(ctx, x, bank, bias, res=None):
        x = x.contiguous(memory_format=torch.channels_last)
        ctx.save_for_backward(x, bank)
        return ops.gconv1x1_nhwc(x, ops.pack_gconv1x1_weights(bank.detach()), bias.detach().contiguous(),
                                 None if res is None else res.contiguous(memory_format=torch.channels_last))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, bank = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        cout, cin = bank.shape[:2]
        dx = dbank = dbias = None
        if ctx.needs_input_grad[0]:
            wt = ops.pack_gconv1x1_weights(bank.detach().reshape(cout, cin).t().contiguous())
            dx = ops.gconv1x1_nhwc(dy, wt, dy.new_zeros(cin))
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dbank, dbias = ops.gconv1x1_wgrad(x, dy)
            dbank = dbank.reshape(bank.shape)
        return (dx, dbank if ctx.needs_input_grad[1] else None, dbias if ctx.needs_input_grad[2] else None,
                dy if len(ctx.needs_input_grad) > 3 and ctx.needs_input_grad[3] else None)


class _ExactQuarterTurns:
    """The group convolutions of this network: the package's layers with a filter bank that is EXACT where the group's rotations are
    quarter turns (num_rotations 1, 2, 4 -- the recipe's C4 and D4).  A quarter turn of a k x k grid, with or without the flip, is a
    permutation of its taps.  `filter_action_matrices` resamples the taps bilinearly in fp32 as the reference does, with a cos(90 deg)
    that is not 0, and comes out up to 4e-7 (k = 3; 7e-7 at k = 5) off that permutation: enough to leave a network of these layers
    equivariant to 4e-7 of its output only, in fp64 as well, where e2cnn's C4 / D4 networks are equivariant to rounding.  Here the
    matrices are rounded to the permutation they stand for.  Other rotation counts: the layer's own bank."""

    def _action_matrices(self, w: torch.Tensor) -> torch.Tensor:
        if 4 % self.num_rotations:
            return super()._action_matrices(w)
        return filter_action_matrices(self.kernel_size, self.num_rotations, self.reflections, w.device).round().to(w.dtype)   # entries 0 / 1


class _Lift(_ExactQuarterTurns, RotationEquivariantConvLift):
    pass


class _Conv(_ExactQuarterTurns, RotationEquivariantConv):
    pass


class _LiftReflect(_ExactQuarterTurns, RotoReflectionEquivariantConvLift):
    pass


class _ConvReflect(_ExactQuarterTurns, RotoReflectionEquivariantConv):
    pass


def _group_layers(group_type: str):
    """(lifting layer, group convolution) of the group."""
    if group_type == "rotation":
        return _Lift, _Conv
    if group_type == "roto-reflection":
        return _LiftReflect, _ConvReflect
    raise ValueError("group_type must be rotation or roto-reflection for now.")


def _is_conv(m: nn.Module) -> bool:
    return hasattr(m, "expanded_weights")


def _plain_conv(conv, x: torch.Tensor) -> torch.Tensor:
    """The layer as F.conv2d on its expanded bank, (B, [fields, |G|,] H, W) -> (B, fields, |G|, H', W'): the layer's own forward
    without its hand-written lifting kernel, so that the plain route is the same ops on every device and dtype."""
    B = x.shape[0]
    if not conv.lifting:
        x = x.flatten(1, 2)
    y = F.conv2d(x, conv.expanded_weights(), stride=conv.stride, padding=conv.padding)
    y = y.reshape(B, conv.out_channels, conv.num_group_elements, y.shape[-2], y.shape[-1])
    if conv.bias is not None:
        y = y + conv.bias[None, :, None, None, None]
    return y


def _plain_chain(mods, x: torch.Tensor, routes: Optional[List[str]]) -> torch.Tensor:
    for m in mods:
        if _is_conv(m):
            x = _plain_conv(m, x)
            if routes is not None:
                routes.append("conv2d")
        else:
            x = m(x)
    return x


class ESCNNWideBottleneck(nn.Module):
    """conv 1 x 1 in -> middle, InnerBN, ReLU; conv k x k middle -> out (padding k // 2), InnerBN, ReLU; conv 1 x 1 out -> in; + x
    (reference :228-298).  Maps are (B, fields, |G|, H, W)."""

    def __init__(self, in_fields: int, middle_fields: int, out_fields: int, kernel_size: int = 3, group_type: str = "rotation",
                 num_rotations: int = 4):
        super().__init__()
        _, conv = _group_layers(group_type)
        self.in_fields, self.middle_fields, self.out_fields, self.kernel_size = in_fields, middle_fields, out_fields, kernel_size
        self.conv_network = nn.Sequential(
            conv(in_fields, middle_fields, 1, num_rotations, device="cpu"),
            _InnerBatchNorm(middle_fields, momentum=0.9),
            nn.ReLU(inplace=True),
            conv(middle_fields, out_fields, kernel_size, num_rotations, padding=kernel_size // 2, device="cpu"),
            _InnerBatchNorm(out_fields, momentum=0.9),
            nn.ReLU(inplace=True),
            conv(out_fields, in_fields, 1, num_rotations, device="cpu"),
        )

    def forward(self, x: torch.Tensor, routes: Optional[List[str]] = None) -> torch.Tensor:
        return _plain_chain(self.conv_network, x, routes) + x

    def _fused(self, net: "ESCNNWRNEquivariantNetwork", h: torch.Tensor, outer_bn: nn.Module, routes: List[str]) -> torch.Tensor:
        """relu(outer_bn(block(h))) on the channels-last map h (batch-norms in eval mode)."""
        c1, bn1, _, c2, bn2, _, c3 = self.conv_network
        u = net._conv1x1(h, c1, bn1, None, None, True, routes)
        u = net._convkxk(u, c2, bn2, True, routes)
        return net._conv1x1(u, c3, None, h, net._affine(outer_bn), True, routes)


class ESCNNWideBasic(nn.Module):
    """conv k x k in -> middle, InnerBN, ReLU; conv k x k middle -> out (neither padded); + shortcut(x), one conv in -> out with kernel
    2 k - 1 (the identity when in == out, which needs k = 1) (reference :301-373).  Maps are (B, fields, |G|, H, W)."""

    def __init__(self, in_fields: int, middle_fields: int, out_fields: int, kernel_size: int = 3, group_type: str = "rotation",
                 num_rotations: int = 4):
        super().__init__()
        _, conv = _group_layers(group_type)
        self.in_fields, self.middle_fields, self.out_fields, self.kernel_size = in_fields, middle_fields, out_fields, kernel_size
        self.conv_network = nn.Sequential(
            conv(in_fields, middle_fields, kernel_size, num_rotations, device="cpu"),
            _InnerBatchNorm(middle_fields, momentum=0.9),
            nn.ReLU(inplace=True),
            conv(middle_fields, out_fields, kernel_size, num_rotations, device="cpu"),
        )
        self.shortcut = None
        if in_fields != out_fields:
            self.shortcut = nn.Sequential(conv(in_fields, out_fields, 2 * kernel_size - 1, num_rotations, device="cpu"))

    def forward(self, x: torch.Tensor, routes: Optional[List[str]] = None) -> torch.Tensor:
        out = _plain_chain(self.conv_network, x, routes)
        return out + (_plain_chain(self.shortcut, x, routes) if self.shortcut is not None else x)

    def _fused(self, net: "ESCNNWRNEquivariantNetwork", h: torch.Tensor, outer_bn: nn.Module, routes: List[str]) -> torch.Tensor:
        """relu(outer_bn(block(h))) on the channels-last map h; the junction (add, affine, ReLU) as torch ops."""
        c1, bn1, _, c2 = self.conv_network
        a = net._convkxk(net._convkxk(h, c1, bn1, True, routes), c2, None, False, routes)
        sc = net._convkxk(h, self.shortcut[0], None, False, routes) if self.shortcut is not None else h
        s, t = net._affine(outer_bn)
        return torch.relu_(a.add_(sc).mul_(s[None, :, None, None]).add_(t[None, :, None, None]))


class ESCNNWRNEquivariantNetwork(nn.Module):
    def __init__(self, in_shape: tuple, out_channels: int = 64, kernel_size: int = 9, group_type: str = "rotation",
                 num_layers: int = 12, num_rotations: int = 4):
        super().__init__()
        lift, conv = _group_layers(group_type)
        if num_layers < 3 or num_layers % 3 != 0:
            raise ValueError(f"num_layers must be a multiple of 3, at least 3 (got {num_layers}): the reference's layer list "
                             "(escnn_networks.py:451-460) indexes past its field types otherwise")
        widen_factor = 2
        self.kernel_size = kernel_size
        self.group_type = group_type
        self.out_channels = out_channels * widen_factor
        self.num_rotations = num_rotations
        self.num_group_elements = num_rotations if group_type == "rotation" else 2 * num_rotations
        n2, n3 = out_channels // 4, out_channels // 4 * widen_factor
        n4, n5 = out_channels // 2 * widen_factor, out_channels * widen_factor

        # same module sequence as the reference ctor (:445-483)
        mods: List[nn.Module] = [lift(in_shape[0], n2, kernel_size, num_rotations, device="cpu"), _InnerBatchNorm(n2, momentum=0.9),
                                 nn.ReLU(inplace=True)]
        rep = num_layers // 3
        rs = [n2] * rep + [n3] * rep + [n4] * rep
        for ridx in range(num_layers - 1):
            block = ESCNNWideBasic if ridx % rep == rep - 1 else ESCNNWideBottleneck
            mods += [block(rs[ridx], rs[ridx + 1], rs[ridx + 1], kernel_size, group_type, num_rotations),
                     _InnerBatchNorm(rs[ridx + 1], momentum=0.9), nn.ReLU(inplace=True)]
        mods.append(conv(n4, n5, kernel_size, num_rotations, device="cpu"))
        self.eqv_network = nn.Sequential(*mods)
        self.last_routes: List[str] = []
        self._cache = DerivedCache()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """A checkpoint of the reference's e2cnn network (escnn_networks.py:376-485) cannot be loaded by key: e2cnn stores a flat
        coefficient vector per layer over its steerable basis (``...weights`` 1-D, ``...basisexpansion...`` / ``...filter``
        buffers), this network stores rotated filter banks.  Say so instead of failing on a shape mismatch."""
        refuse_e2cnn_state_dict(
            state_dict, prefix + "eqv_network.", "ESCNNWRNEquivariantNetwork",
            "equiadapt_amd.ESCNNWRNEquivariantNetwork parameterises its layers by rotated filter banks and cannot load it by key.",
            (".expanded_bias",))
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # -- fused route: folded operands, kept in self._cache under the layer; what is built from a bank under (layer, tag) -------------
    def _fold(self, conv, bn) -> Tuple[torch.Tensor, torch.Tensor]:
        """Channels-last filter bank and per-channel bias of ``bn(conv(.))`` in eval mode (bn None: of conv)."""
        def build():
            bank = conv.expanded_weights()
            bias = conv.bias if conv.bias is not None else bank.new_zeros(conv.out_channels)
            if bn is not None:
                scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)                  # per field
                bias = (bias - bn.running_mean) * scale + bn.bias
                bank = bank * scale.repeat_interleave(conv.num_group_elements)[:, None, None, None]
            return bank.contiguous(memory_format=torch.channels_last), bias.repeat_interleave(conv.num_group_elements).contiguous()

        norm = () if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        return self._cache.get(conv, (conv.weights, conv.bias, *norm), build)

    def _affine(self, bn) -> Tuple[torch.Tensor, torch.Tensor]:
        """(s, t) per channel of an InnerBatchNorm in eval mode."""
        return self._cache.get(bn, (bn.weight, bn.bias, bn.running_mean, bn.running_var),
                               lambda: tuple(torch.stack(bn_eval_affine(bn)).repeat_interleave(self.num_group_elements, dim=1)))

    def _conv1x1(self, h, conv, bn, res, affine, relu: bool, routes: List[str]) -> torch.Tensor:
        """act(bn(conv(h)) [+ res]), act = [relu] o affine, for a 1 x 1 layer on the channels-last map h: one launch of
        eqa_gconv1x1_nhwc where it takes the shape, else the library's convolution and torch ops."""
        bank, bias = self._fold(conv, bn)
        cout, cin = bank.shape[:2]
        s, t = affine if affine is not None else (None, None)
        if ops.gconv1x1_supported(h.shape[0] * h.shape[2] * h.shape[3], cin, cout):
            wpk = self._cache.derived(conv, (conv, "gconv1x1"), lambda: ops.pack_gconv1x1_weights(bank))
            routes.append("gconv1x1" if res is None else "gconv1x1+junction")
            return ops.gconv1x1_nhwc(h.contiguous(memory_format=torch.channels_last), wpk, bias,
                                     None if res is None else res.contiguous(memory_format=torch.channels_last), s, t, relu)
        routes.append("lib")
        z = F.conv2d(h, bank, bias)
        if res is not None:
            z = z.add_(res)
        if s is not None:
            z = z.mul_(s[None, :, None, None]).add_(t[None, :, None, None])
        return torch.relu_(z) if relu else z

    def _convkxk(self, h, conv, bn, relu: bool, routes: List[str]) -> torch.Tensor:
        """[relu](bn(conv(h))) for a k x k layer (stride 1, the layer's zero padding) on the channels-last map h: the FFT convolution
        ("fft5" / "fftk") or Winograd ("wino") where their own rules admit the padded map, else the library's convolution ("lib")."""
        bank, bias = self._fold(conv, bn)
        cout, cin = bank.shape[:2]
        k, pad = conv.kernel_size, conv.padding
        hp = F.pad(h, (pad, pad, pad, pad)) if pad else h
        hp = hp.contiguous(memory_format=torch.channels_last)
        if k == 5 and fftconv.applicable(hp, cin, cout):
            routes.append("fft5")
            return fftconv.conv5x5(hp, self._cache.derived(conv, (conv, "fft"), lambda: fftconv.spectra_for_k(bank)), bias, relu)
        if k != 5 and fftconv.applicable_k(hp.shape, cin, cout, k, hp.device):
            routes.append("fftk")
            return fftconv.conv_kxk(hp, self._cache.derived(conv, (conv, "fft"), lambda: fftconv.spectra_for_k(bank)), k, bias, relu)
        if k == 5 and winograd.applicable(hp, cin, cout):
            m = winograd.tile_for(hp)
            routes.append("wino")
            return winograd.conv5x5(hp, self._cache.derived(conv, (conv, "wino", m), lambda: winograd.transform_filters(bank, m)), bias, relu)
        routes.append("lib")
        y = F.conv2d(hp, bank, bias)
        return torch.relu_(y) if relu else y

    def _fused_ok(self, x: torch.Tensor) -> bool:
        if self.training or torch.is_grad_enabled() or os.environ.get("EQA_WRN_KERNEL", "1") == "0":
            return False
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and self.eqv_network[0].weights.dtype == torch.float32):
            return False
        return all(not m.training and m.running_mean is not None for m in self.modules() if isinstance(m, _InnerBatchNorm))

    def _forward_fused(self, x: torch.Tensor, routes: List[str]) -> torch.Tensor:
        mods = list(self.eqv_network)
        stem, tail = mods[0], mods[-1]
        h = x.contiguous(memory_format=torch.channels_last)
        bank, bias = self._fold(stem, mods[1])
        k = stem.kernel_size
        if stem.mfma_lifting_ok(h):
            narrow = ops.lift_conv_supported(bank.shape[1], k, k, bank.shape[0])
            wpk = self._cache.derived(stem, (stem, "lift"), lambda: (ops.pack_lift_weights if narrow else ops.pack_lift_weights_wide)(bank))
            routes.append("lift" if narrow else "lift_wide")
            h = (ops.lift_conv_nhwc if narrow else ops.lift_conv_wide)(h, wpk, bias, True, k, k)
        else:
            routes.append("lib")
            h = torch.relu_(F.conv2d(h, bank, bias))
        for i in range(3, len(mods) - 1, 3):                      # (block, InnerBatchNorm, ReLU)
            h = mods[i]._fused(self, h, mods[i + 1], routes)
        if tail.supports_linear_tail():
            routes.append("window_sums")
            return conv_then_group_pool(h, tail)
        routes.append("lib")
        bank, bias = self._fold(tail, None)
        y = F.conv2d(h, bank, bias)
        return group_pool(y.reshape(y.shape[0], tail.out_channels, self.num_group_elements, y.shape[-2], y.shape[-1]))

    # -- training route --------------------------------------------------------------------------------------------------------
    def _train_ok(self, x: torch.Tensor) -> bool:
        """The entry rule of `_forward_training`, from shapes and flags alone: training mode or gradients enabled, EQA_WRN_KERNEL != 0,
        fp32 input and weights on the device, stride 1 and channel counts on the multiples of 4 everywhere, and at least one
        bottleneck 1 x 1 layer that both eqa_gconv1x1_nhwc and eqa_gconv1x1_wgrad take at this input."""
        if not (self.training or torch.is_grad_enabled()) or os.environ.get("EQA_WRN_KERNEL", "1") == "0":
            return False
        w = self.eqv_network[0].weights
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and w.is_cuda and w.dtype == torch.float32):
            return False
        E = self.num_group_elements
        convs = [m for m in self.modules() if _is_conv(m)]
        if any(c.stride != 1 or (c.out_channels * E) % 4 for c in convs):
            return False
        mods = list(self.eqv_network)
        B, (H, W) = x.shape[0], x.shape[-2:]
        H, W = (v + 2 * mods[0].padding - mods[0].kernel_size + 1 for v in (H, W))
        admitted = False
        for block in mods[3:-1:3]:
            if min(H, W) < 1:
                return False
            if isinstance(block, ESCNNWideBottleneck):
                for c in (block.conv_network[0], block.conv_network[6]):
                    sizes = (B * H * W, c.in_channels * E, c.out_channels * E)
                    admitted = admitted or (ops.gconv1x1_supported(*sizes) and ops.gconv1x1_wgrad_supported(*sizes))
            else:
                H, W = H - 2 * (block.kernel_size - 1), W - 2 * (block.kernel_size - 1)
        return admitted and min(H, W) >= 1

    def _forward_training(self, x: torch.Tensor, routes: List[str]) -> torch.Tensor:
        """Same layers as ``self.eqv_network`` + group pooling with autograd, channels-last (B, fields * |G|, H, W) throughout.  Per
        layer, from shapes alone: a 1 x 1 layer on `GConv1x1Function` ("gconv1x1"; a bottleneck's second one with the block input as
        the residual, "gconv1x1+junction") where both kernels take it; a k x k layer, zero-padded by F.pad where the layer is
        padded, on ``winograd.Conv5x5Function`` ("wino") or ``fftconv.ConvKxKFunction`` ("fftk") where their rules admit the map;
        the stem on `LiftConvFunction` ("lift" / "lift_wide"); else the library's convolution ("lib").  Every InnerBatchNorm + ReLU
        is one `InnerBnReluDropout` with p = 0 (batch statistics and the running-statistics update in training mode, running
        statistics in eval mode; EQA_TRAIN_FUSED_BN=0: op by op).  A k x k layer's bias goes to the batch-norm behind it, where it
        only shifts the mean.  The last convolution + group mean are window sums + a GEMV ("window_sums") where the tail is linear
        and the map fits, else convolution + group_pool ("lib")."""
        mods = list(self.eqv_network)
        stem, tail = mods[0], mods[-1]
        E = self.num_group_elements
        fused_bn = os.environ.get("EQA_TRAIN_FUSED_BN", "1") != "0"
        nhwc = torch.channels_last
        handed: List[torch.Tensor] = []      # biases handed to a batch-norm: kept in the graph (see the end)

        def bn_relu(h, bn, conv_bias):
            if conv_bias is not None:
                handed.append(conv_bias.sum())
            if fused_bn and h.is_contiguous(memory_format=nhwc):
                return InnerBnReluDropout.apply(h, bn.weight, bn.bias, bn, E, conv_bias, 0.0, False, None)
            return torch.relu(ESCNNEquivariantNetwork._inner_bn(h, bn, E, conv_bias))

        def one_by_one(h, conv, res):
            bank = conv.expanded_weights()
            cout, cin = bank.shape[:2]
            bias = bank.new_zeros(cout) if conv.bias is None else conv.bias.repeat_interleave(E)
            sizes = (h.shape[0] * h.shape[2] * h.shape[3], cin, cout)
            if ops.gconv1x1_supported(*sizes) and ops.gconv1x1_wgrad_supported(*sizes):
                routes.append("gconv1x1" if res is None else "gconv1x1+junction")
                return GConv1x1Function.apply(h, bank, bias, res)
            routes.append("lib")
            y = F.conv2d(h, bank.contiguous(memory_format=nhwc), bias)
            return y if res is None else y + res

        def k_by_k(h, conv):                 # without the layer's bias
            bank = conv.expanded_weights()
            cout, cin = bank.shape[:2]
            k, pad = conv.kernel_size, conv.padding
            hp = (F.pad(h, (pad, pad, pad, pad)) if pad else h).contiguous(memory_format=nhwc)
            if k == 5 and winograd.applicable(hp, cin, cout):
                routes.append("wino")
                return winograd.Conv5x5Function.apply(hp, bank, winograd.tile_for(hp), False)
            if k != 5 and fftconv.applicable_k(hp.shape, cin, cout, k, hp.device):
                routes.append("fftk")
                return fftconv.ConvKxKFunction.apply(hp, bank)
            routes.append("lib")
            return F.conv2d(hp, bank.contiguous(memory_format=nhwc))

        h = x.contiguous(memory_format=nhwc)
        bank = stem.expanded_weights()
        lift = ESCNNEquivariantNetwork._lift_kernel(stem, bank, h)
        if lift is not None:
            routes.append("lift" if lift == "narrow" else "lift_wide")
            h = LiftConvFunction.apply(h, bank, False)
        else:
            routes.append("lib")
            h = F.conv2d(h, bank.contiguous(memory_format=nhwc), padding=stem.padding)
        h = bn_relu(h, mods[1], stem.bias)
        for i in range(3, len(mods) - 1, 3):                      # (block, InnerBatchNorm, ReLU)
            block, outer = mods[i], mods[i + 1]
            if isinstance(block, ESCNNWideBottleneck):
                c1, bn1, _, c2, bn2, _, c3 = block.conv_network
                u = bn_relu(one_by_one(h, c1, None), bn1, None)
                u = bn_relu(k_by_k(u, c2), bn2, c2.bias)
                h = bn_relu(one_by_one(u, c3, h), outer, None)
            else:
                c1, bn1, _, c2 = block.conv_network
                a = k_by_k(bn_relu(k_by_k(h, c1), bn1, c1.bias), c2)
                bias = c2.bias
                if block.shortcut is not None:
                    sc = block.shortcut[0]
                    a = a + k_by_k(h, sc)
                    bias = sc.bias if bias is None else bias if sc.bias is None else bias + sc.bias
                else:
                    a = a + h
                h = bn_relu(a, outer, bias)
        k, O = tail.kernel_size, tail.out_channels
        Bn, _, H, W = h.shape
        bank = tail.expanded_weights()
        if tail.supports_linear_tail() and min(H, W) >= 2 * k - 1 and H * W <= 12288 and Bn <= 65535:
            routes.append("window_sums")
            S = WindowSumsFunction.apply(h.contiguous(memory_format=nhwc), k)                      # (B, C, k, k) fp64
            weff = bank.reshape(O, E, -1).double().sum(0)                                          # (E, C*k*k), differentiable
            scale = 1.0 / float(O * (H - k + 1) * (W - k + 1))
            if E <= 16 and os.environ.get("EQA_WS_TABLE_KERNEL", "1") != "0":
                act = WindowSumsLinearFn.apply(S.flatten(1), weff, scale)
            else:
                act = S.flatten(1) @ weff.t() * scale
            if tail.bias is not None:
                act = act + tail.bias.double().mean()
        else:
            routes.append("lib")
            y = F.conv2d(h, bank.contiguous(memory_format=nhwc), None if tail.bias is None else tail.bias.repeat_interleave(E),
                         padding=tail.padding)
            act = group_pool(y.reshape(Bn, O, E, y.shape[-2], y.shape[-1]).contiguous())
        # a bias in front of a batch-norm with batch statistics cancels (zero gradient): it stays in the graph with that exact zero,
        # so that every parameter has a gradient tensor and DistributedDataParallel counts it as used
        if handed:
            act = act + 0.0 * torch.stack(handed).sum()
        return act.float()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        routes: List[str] = []
        if self._fused_ok(x):
            out = self._forward_fused(x, routes)
        elif self._train_ok(x):
            out = self._forward_training(x, routes)
        else:
            h = x
            for m in self.eqv_network:
                if isinstance(m, (ESCNNWideBottleneck, ESCNNWideBasic)):
                    h = m(h, routes)
                else:
                    h = _plain_chain([m], h, routes)
            out = group_pool(h)
        self.last_routes = routes
        return out
