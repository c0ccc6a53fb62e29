"""ESCNNEquivariantNetwork: regular-representation G-CNN canonicalization network.

Reference: equiadapt/images/canonicalization_networks/escnn_networks.py:8-117, built there from e2cnn
``R2Conv`` + ``InnerBatchNorm(momentum=0.9)`` + ``ReLU`` + ``PointwiseDropout(0.5)``.

e2cnn is not available to this build and its steerable-basis expansion is not restated here
(SURVEY.md section 8c).  This class keeps the reference's constructor, tensor shapes, layer order, FLOPs and
output contract ((B, G) activations = mean over fields and space), and parameterises every conv by a
rotated filter bank (trivial->regular lifting, then regular->regular group convs, all k x k, no padding).
InnerBatchNorm over a regular field shares statistics across the G channels of the field, i.e. it is
BatchNorm3d over (B, fields, G, H, W); PointwiseDropout is element-wise dropout.
Weights trained with e2cnn can be brought in through their exported dense form
(``R2Conv.export()`` -> Conv2d, ``InnerBatchNorm.export()`` -> BatchNorm2d): ``load_exported_dense``.
"""
import os
from typing import List, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from equiadapt_amd.images.canonicalization_networks.custom_group_equivariant_layers import (
    RotationEquivariantConv,
    RotationEquivariantConvLift,
    RotoReflectionEquivariantConv,
    RotoReflectionEquivariantConvLift,
)
from equiadapt_amd import ops
from equiadapt_amd.common.derived import DerivedCache, bn_eval_affine, refuse_e2cnn_state_dict
from equiadapt_amd.common.utils import update_running_stats
from equiadapt_amd.images.canonicalization_networks import fftconv, winograd
from equiadapt_amd.images.canonicalization_networks.pooling import (
    WindowSumsFunction,
    WindowSumsLinearFn,
    conv_then_group_pool,
    group_pool,
    sums_tail_operands,
    window_grad_table,
    window_sums_to_activations,
)
from equiadapt_amd.images.canonicalization_networks.steerable_networks import ESCNNSteerableNetwork  # noqa: F401  (reference: same module)


class _InnerBatchNorm(nn.BatchNorm3d):
    """Per-field batch norm over (batch, group, space) of a (B, fields, G, H, W) map."""


class LiftConvFunction(torch.autograd.Function):
    """Training counterpart of the lifting convolution in `_forward_inference`: forward on the fp32-MFMA kernel
    (`eqa_lift_conv_nhwc`, 0.71 ms at the headline shape; wide / single-channel filters: `eqa_lift_conv_wide`), filter gradient on
    the matrix cores too (`eqa_lift_conv_wgrad_nhwc` / `eqa_lift_conv_wide_wgrad`; shapes neither takes: the framework's
    convolution-weight-gradient).  The input image needs no gradient in the canonicalizer; if asked for, it is the framework's."""

    @staticmethod
    def forward(ctx, x, bank, with_stats=False):
        """with_stats: also return the fp64 partial sums (rows, Cout, 2) of the output's per-channel sum / sum of squares, taken in the
        kernel's epilogue (eqa_lift_conv_nhwc_stats) -- the batch-norm behind the layer then skips its own pass over the map."""
        ctx.save_for_backward(x, bank)
        k = bank.shape[-1]
        if not ops.lift_conv_supported(bank.shape[1], bank.shape[-2], k, bank.shape[0]):      # wide / single-channel filters
            if with_stats:
                raise ValueError("LiftConvFunction: with_stats needs a shape eqa_lift_conv_nhwc_stats takes (gate on ops.lift_conv_supported)")
            return ops.lift_conv_wide(x, ops.pack_lift_weights_wide(bank.detach()), None, False, bank.shape[-2], k)
        wpk = ops.pack_lift_weights(bank.detach())
        if with_stats:
            y, part = ops.lift_conv_nhwc_stats(x, wpk, bank.shape[-2], k)
            ctx.mark_non_differentiable(part)
            return y, part
        return ops.lift_conv_nhwc(x, wpk, None, False, bank.shape[-2], k)

    @staticmethod
    def backward(ctx, dy, *_):
        x, bank = ctx.saved_tensors
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.nn.grad.conv2d_input(x.shape, bank, dy) if ctx.needs_input_grad[0] else None
        dbank = None
        if ctx.needs_input_grad[1]:
            kh, kw = bank.shape[-2], bank.shape[-1]
            if ops.lift_conv_wgrad_supported(x, bank.shape[0], kh, kw):
                dbank = ops.lift_conv_wgrad_nhwc(x, dy, kh, kw)            # fp32 MFMA, 0.8 ms where MIOpen's solvers take 3.1
            elif ops.lift_conv_wide_supported(bank.shape[1], kh, kw, bank.shape[0]) and x.shape[0] > 0:
                dbank = ops.lift_conv_wide_wgrad(x, dy, kh, kw)            # the wide / single-channel filters (tutorial k = 9)
            else:
                dbank = torch.nn.grad.conv2d_weight(x, bank.shape, dy)
        return dx, dbank, None


def _moments(s1, s2, n, bn, conv_bias):
    """Per-field sum and sum of squares (fp64) over n elements -> batch mean and biased variance (fp32), the running statistics updated
    like nn.BatchNorm3d (momentum, unbiased variance).  The preceding convolution's bias only shifts the mean (it cancels in the
    normalised output), so it enters the running mean and nowhere else."""
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    with torch.no_grad():
        full_mean = mean if conv_bias is None else mean + conv_bias.double()
        update_running_stats(bn, full_mean, var * (n / max(n - 1, 1)))
    return mean.float(), var.float()


def _block_affine(h, weight, bias, bn, E, conv_bias, part):
    """InnerBatchNorm of the channels-last (B, fields*E, H, W) map h as a per-channel affine map: (mean_c, rstd_c, scale, shift,
    batch_stats), each vector repeated over the E channels of its field.  Batch statistics per field over (batch, group, space) in
    fp64, from part -- the (rows, C, 2) fp64 partial sums of h's per-channel sum / sum of squares, when the kernel that produced h
    took them on the way out (LiftConvFunction with_stats, the FFT convolution's inverse transform) -- or from one pass over h here;
    a batch-norm in eval mode: its running statistics."""
    Bn, C, H, W = h.shape
    Fd = C // E
    batch_stats = bool(bn.training or bn.running_mean is None)
    if batch_stats:
        sums = (ops.inner_bn_stats(h) if part is None else part).sum(0).view(Fd, E, 2).sum(1)              # (fields, 2) fp64
        mean, var = _moments(sums[:, 0], sums[:, 1], Bn * H * W * E, bn, None if conv_bias is None else conv_bias.detach())
    else:
        mean = bn.running_mean if conv_bias is None else bn.running_mean - conv_bias.detach()
        var = bn.running_var
    rstd = torch.rsqrt(var + bn.eps)
    scale = weight.detach() * rstd
    mean_c, rstd_c, scale, shift = torch.stack([mean, rstd, scale, bias.detach() - mean * scale]).repeat_interleave(E, dim=1)
    return mean_c, rstd_c, scale, shift, batch_stats                         # (rows of one contiguous (4, C) tensor)


def _dropout_draw(p, drop_training):
    """(p_eff, seed) of the block's dropout mask, a hash of (seed, element index): the seed is drawn from torch's CPU generator, so
    torch.manual_seed reproduces the mask; no draw where nothing is dropped."""
    p_eff = float(p) if drop_training else 0.0
    return p_eff, (int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_eff > 0 else 0)


def _block_backward(ctx, g, k=0):
    """The hidden block's gradients for the eight inputs its two Functions share (h, weight, bias, bn, E, conv_bias, p, drop_training),
    from what the forward left in ctx.  g, k: the upstream gradient as `ops.inner_bn_bwd_reduce` takes it (k = 0: a channels-last
    map; k > 0: the window sums' class table)."""
    h, weight, mean_c, rstd_c, scale, shift = ctx.saved_tensors
    E = ctx.E
    Bn, C, H, W = h.shape
    Fd = C // E
    part = ops.inner_bn_bwd_reduce(g, h, mean_c, rstd_c, scale, shift, ctx.p, ctx.seed, k)
    sums = part.sum(0).view(Fd, E, 2).sum(1)                                 # per field: sum g, sum g*xhat
    dbias, dweight = sums[:, 0].float(), sums[:, 1].float()
    if ctx.batch_stats:
        bd = (sums / (Bn * H * W * E)).float().t()                           # per field: mean of g, of g*xhat
    else:                                                                    # running statistics are constants
        bd = torch.zeros(2, Fd, device=h.device)
    a, b, d = torch.cat([(weight * rstd_c.view(Fd, E)[:, 0])[None], bd]).repeat_interleave(E, dim=1)
    dh = ops.inner_bn_bwd_apply(g, h, mean_c, rstd_c, a, b, d, scale, shift, ctx.p, ctx.seed, k)
    # With batch statistics the convolution bias cancels in the normalised output (zero gradient).  With running statistics
    # (frozen batch-norm under autograd) it does not: out = scale * (h + conv_bias - running_mean) + ..., so
    # d conv_bias = per-field sum of dh, as the op-by-op path and the reference propagate it.
    # The zero is returned as a tensor, not as None: the reference and the op-by-op path leave an exact-zero .grad on the
    # bias, which weight decay then acts on and which DistributedDataParallel needs to count the parameter as used.
    dconv_bias = None
    if ctx.has_conv_bias and ctx.needs_input_grad[5]:
        if ctx.batch_stats:
            dconv_bias = torch.zeros(Fd, dtype=h.dtype, device=h.device)
        else:
            dconv_bias = dh.sum(dim=(0, 2, 3), dtype=torch.float64).view(Fd, E).sum(1).float()
    return dh, dweight, dbias, None, None, dconv_bias, None, None


class InnerBnReluDropout(torch.autograd.Function):
    """dropout(relu(InnerBatchNorm(h))) on a channels-last (B, fields*E, H, W) map, forward and backward on the fused
    kernels of csrc/batchnorm.hip (eqa_bn_*): statistics and affine map by `_block_affine`, mask seed by `_dropout_draw`; the
    backward (`_block_backward`) recomputes "kept and positive" from h, the affine map and that seed instead of reading y (one map
    less per pass)."""

    @staticmethod
    def forward(ctx, h, weight, bias, bn, E, conv_bias, p, drop_training, part=None):
        mean_c, rstd_c, scale, shift, batch_stats = _block_affine(h, weight, bias, bn, E, conv_bias, part)
        p_eff, seed = _dropout_draw(p, drop_training)
        ctx.save_for_backward(h, weight, mean_c, rstd_c, scale, shift)       # not y: see above
        ctx.E, ctx.p, ctx.seed, ctx.batch_stats, ctx.has_conv_bias = E, p_eff, seed, batch_stats, conv_bias is not None
        return ops.inner_bn_relu_dropout(h, scale, shift, p_eff, seed)

    @staticmethod
    def backward(ctx, gy):
        return _block_backward(ctx, gy.contiguous(memory_format=torch.channels_last)) + (None,)


class InnerBnReluDropoutWindowSums(torch.autograd.Function):
    """The last hidden block and the window sums that consume it, S = window_sums(dropout(relu(InnerBatchNorm(h))), k), without
    the block's output ever existing: the forward applies the affine map, the ReLU and the dropout mask while the window-sum
    kernel loads h (eqa_window_sums_nhwc_act); the backward reads the upstream gradient from the window sums' (2k-1) x (2k-1) class
    table (eqa_bn_bwd_*_wsgrad) instead of an expanded map.  Against InnerBnReluDropout + WindowSumsFunction at the headline shape
    (256 x 88 x 88 x 256): one 2.2 GB map less written and read in the forward, one less written and two fewer reads in the backward
    (-2.0 ms of the 29.7 ms training step).  Same statistics, same mask, same arithmetic per element: everything but the launches
    is InnerBnReluDropout's."""

    @staticmethod
    def forward(ctx, h, weight, bias, bn, E, conv_bias, p, drop_training, k, part=None):
        mean_c, rstd_c, scale, shift, batch_stats = _block_affine(h, weight, bias, bn, E, conv_bias, part)
        p_eff, seed = _dropout_draw(p, drop_training)
        ctx.save_for_backward(h, weight, mean_c, rstd_c, scale, shift)
        ctx.E, ctx.p, ctx.seed, ctx.batch_stats, ctx.has_conv_bias, ctx.k = E, p_eff, seed, batch_stats, conv_bias is not None, k
        return ops.window_sums_nhwc_act(h, scale, shift, p_eff, seed, k)

    @staticmethod
    def backward(ctx, dS):
        h = ctx.saved_tensors[0]
        return _block_backward(ctx, window_grad_table(dS, h.shape[-2], h.shape[-1], ctx.k), ctx.k) + (None, None)


class _DenseConv(nn.Module):
    """An exported dense convolution (e2cnn ``R2Conv.export()`` -> nn.Conv2d over fields x group channels, channel index =
    field * |G| + element) behind the interface the inference fast path expects from a group convolution."""

    def __init__(self, conv: nn.Conv2d, num_group_elements: int, lifting: bool):
        super().__init__()
        if conv.kernel_size[0] != conv.kernel_size[1] or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1] \
                or conv.groups != 1 or conv.dilation != (1, 1) or isinstance(conv.padding, str):
            raise ValueError("exported convolutions must be square, ungrouped, undilated, with numeric padding")
        if conv.out_channels % num_group_elements:
            raise ValueError(f"{conv.out_channels} output channels are not a whole number of regular fields of size {num_group_elements}")
        self.conv = conv
        self.num_group_elements = num_group_elements
        self.lifting = lifting
        self.kernel_size, self.stride, self.padding = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        self.out_channels = conv.out_channels // num_group_elements          # fields, like the group convolutions
        self._cache = DerivedCache()

    @property
    def weights(self):
        return self.conv.weight

    @property
    def bias(self):
        return self.conv.bias                                                # per CHANNEL (fields x |G|)

    def expanded_weights(self) -> torch.Tensor:
        return self.conv.weight

    def mean_response_weights(self) -> torch.Tensor:
        w = self.conv.weight
        return self._cache.get("weff", (w,), lambda: w.detach().view(self.out_channels, self.num_group_elements, -1).double().sum(0))

    def mean_bias_value(self):
        """Per-ELEMENT mean of the bias over the fields, (|G|,) fp64: an exported bias is constant within a regular field for an
        equivariant layer, but nothing here relies on that."""
        b = self.conv.bias
        if b is None:
            return 0.0

        def build():
            m = b.detach().double().view(self.out_channels, self.num_group_elements).mean(0)
            return float(m[0].item()) if bool((m == m[0]).all().item()) else m

        return self._cache.get("bias_mean", (b,), build)

    def supports_linear_tail(self) -> bool:
        return self.stride == 1 and self.padding == 0 and self.kernel_size <= ops.MAX_WINDOW_K

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.conv(x)


class ESCNNEquivariantNetwork(nn.Module):
    def __init__(self, in_shape: tuple, out_channels: int, kernel_size: int, group_type: str = "rotation",
                 num_rotations: int = 4, num_layers: int = 1):
        super().__init__()
        self.in_channels = in_shape[0]
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.group_type = group_type
        self.num_rotations = num_rotations
        if group_type == "rotation":
            lift, conv = RotationEquivariantConvLift, RotationEquivariantConv
        elif group_type == "roto-reflection":
            lift, conv = RotoReflectionEquivariantConvLift, RotoReflectionEquivariantConv
        else:
            raise ValueError("group_type must be rotation or roto-reflection for now.")
        self.num_group_elements = num_rotations if group_type == "rotation" else 2 * num_rotations

        def block() -> List[nn.Module]:
            return [_InnerBatchNorm(out_channels, momentum=0.9), nn.ReLU(inplace=True), nn.Dropout(p=0.5)]

        # same module sequence as the reference ctor (:67-91): conv, [bn relu drop, conv] x (L-2), bn relu drop, conv
        mods: List[nn.Module] = [lift(self.in_channels, out_channels, kernel_size, num_rotations, device="cpu")]
        mods += block()
        for _ in range(num_layers - 2):
            mods.append(conv(out_channels, out_channels, kernel_size, num_rotations, device="cpu"))
            mods += block()
        mods.append(conv(out_channels, out_channels, kernel_size, num_rotations, device="cpu"))
        self.eqv_network = nn.Sequential(*mods)
        self._dense: Sequence = ()
        self._cache = DerivedCache()
        # The inference tail in one launch (eqa_window_sums_tail).  A canonicalizer that wants the element with the activations sets
        # `element_tables` = (rotation, reflection or None) device tables around its call; where the fused tail ran, `last_element` =
        # (the activations tensor returned, index, rotation, reflection or None), else None.  `last_routes`: what the last
        # inference call ran -- one word per layer, "bound:<where the fused lifting kernel's pixel bound came from>" behind a
        # fused lifting layer, "tail:<launches of the tail>" at the end.
        self.element_tables = None
        self.last_element = None
        self.last_routes: List[str] = []

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """A checkpoint of the reference's e2cnn network (escnn_networks.py:48-91) cannot be loaded by key: e2cnn stores a flat
        coefficient vector per layer over its steerable basis (``...weights`` 1-D, ``...basisexpansion...`` / ``...filter``
        buffers), this network stores rotated filter banks.  Say so instead of failing on a shape mismatch."""
        refuse_e2cnn_state_dict(
            state_dict, prefix + "eqv_network.", "ESCNNEquivariantNetwork",
            "equiadapt_amd.ESCNNEquivariantNetwork parameterises its layers by rotated filter banks and cannot load it by key; "
            "export the trained layers on the e2cnn side (R2Conv.export() -> nn.Conv2d, InnerBatchNorm.export() -> nn.BatchNorm2d) "
            "and pass them to load_exported_dense(convs, norms).", (".expanded_bias",))
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def load_exported_dense(self, convs: Sequence[nn.Conv2d], norms: Sequence[nn.BatchNorm2d]) -> None:
        """Use exported dense layers (lists in network order) instead of the filter-bank parameterisation: the bridge for
        weights trained with e2cnn, whose steerable-basis parameters cannot be loaded by key (``R2Conv.export()`` ->
        ``nn.Conv2d`` over fields x |G| channels, ``InnerBatchNorm.export()`` -> ``nn.BatchNorm2d``; reference network:
        escnn_networks.py:48-91).  Inference runs through the same fast path as the filter-bank form (FFT / Winograd / MFMA
        lifting layer, folded batch-norms, linearised last layer); with autograd the plain modules are used."""
        n_conv = sum(1 for m in self.eqv_network if hasattr(m, "expanded_weights"))
        if len(convs) != n_conv or len(norms) != n_conv - 1:
            raise ValueError(f"expected {n_conv} convs and {n_conv - 1} norms")
        E = self.num_group_elements
        cin = self.in_channels
        for i, cv in enumerate(convs):
            if cv.in_channels != cin:
                raise ValueError(f"exported conv {i} takes {cv.in_channels} channels, the network feeds it {cin}")
            cin = cv.out_channels
        for i, bn in enumerate(norms):
            if bn.num_features != convs[i].out_channels:
                raise ValueError(f"exported norm {i} has {bn.num_features} features, conv {i} produces {convs[i].out_channels}")
        self._dense = (nn.ModuleList(_DenseConv(cv, E, i == 0) for i, cv in enumerate(convs)), nn.ModuleList(norms))
        self._cache.clear()

    def export_dense(self):
        """(convs, norms): this network's layers in the exported dense form -- expanded filter banks as ``nn.Conv2d`` (bias per
        channel), InnerBatchNorm as ``nn.BatchNorm2d`` with every per-field quantity repeated |G| times -- i.e. what
        ``load_exported_dense`` takes.  Eval-mode equivalent of the filter-bank network."""
        E = self.num_group_elements
        convs, norms = [], []
        with torch.no_grad():
            for m in self.eqv_network:
                if hasattr(m, "expanded_weights"):
                    bank = m.expanded_weights().detach()
                    cv = nn.Conv2d(bank.shape[1], bank.shape[0], m.kernel_size, m.stride, m.padding, bias=m.bias is not None)
                    cv = cv.to(bank.device)
                    cv.weight.copy_(bank)
                    if m.bias is not None:
                        cv.bias.copy_(m.bias.detach().repeat_interleave(E))
                    convs.append(cv)
                elif isinstance(m, _InnerBatchNorm):
                    bn = nn.BatchNorm2d(m.num_features * E, eps=m.eps, momentum=m.momentum).to(m.weight.device)
                    for name in ("weight", "bias", "running_mean", "running_var"):
                        getattr(bn, name).copy_(getattr(m, name).repeat_interleave(E))
                    norms.append(bn.eval())
        return convs, norms

    def _layers(self):
        """(convs, norms) the forward paths iterate over: the exported dense layers if loaded, else the group convolutions."""
        if self._dense:
            return list(self._dense[0]), list(self._dense[1])
        mods = list(self.eqv_network)
        return [m for m in mods if hasattr(m, "expanded_weights")], [m for m in mods if isinstance(m, _InnerBatchNorm)]

    # -- inference fast path ------------------------------------------------------------------------------------
    def _folded(self, conv, bn):
        """Filter bank and bias of ``bn(conv(.))`` in eval mode: the per-field affine of the batch-norm is folded into
        the bank (one conv, no separate bias / normalisation passes over the feature map).  Cached under conv; what is built from
        the bank (transformed filters, packed weights) is cached beside it under ``(conv, tag)``: ``self._cache.derived``."""
        def build():
            E = conv.num_group_elements
            scale, shift = bn_eval_affine(bn)                                      # per field (per channel: exported form)
            b = conv.bias if conv.bias is not None else torch.zeros_like(scale)
            bias = b * scale + shift
            if not isinstance(conv, _DenseConv):
                scale, bias = scale.repeat_interleave(E), bias.repeat_interleave(E)
            bank = conv.expanded_weights() * scale[:, None, None, None]
            # channels-last: MIOpen's fp32 implicit-GEMM kernels are NHWC; keeping the bank (and the activations) in that
            # layout removes the NCHW<->NHWC transposes around every convolution
            return bank.contiguous(memory_format=torch.channels_last), bias.contiguous()

        return self._cache.get(conv, (conv.weights, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var), build)

    @staticmethod
    def _plain_5x5(conv) -> bool:
        return not conv.lifting and conv.kernel_size == 5 and conv.stride == 1 and conv.padding == 0

    @staticmethod
    def _lift_kernel(conv, bank, h, narrow_unchecked: bool = False):
        """Which hand-written lifting kernel takes conv on the map h: "narrow" (the fp32-MFMA implicit GEMM eqa_lift_conv_nhwc and the
        forms built on it), "wide" (eqa_lift_conv_wide: 7 x 7 / 9 x 9 over RGB -- the reference tutorial's k = 9 -- and grayscale), or
        None (the library).  ``narrow_unchecked``: the training forward, where `_training_fast_path_ok` has established stride 1 and
        no padding for every layer, takes the narrow kernel on the shape test alone."""
        if not conv.lifting or os.environ.get("EQA_LIFT_MFMA", "1") == "0":
            return None
        k, (cout, cin) = conv.kernel_size, bank.shape[:2]
        unit = conv.stride == 1 and conv.padding == 0
        if (unit or narrow_unchecked) and ops.lift_conv_supported(cin, k, k, cout):
            return "narrow"
        if (unit and h.is_contiguous(memory_format=torch.channels_last) and h.shape[-2] >= k and h.shape[-1] >= k
                and ops.lift_conv_wide_supported(cin, k, k, cout)):
            return "wide"
        return None

    def _route(self, i, h, bank, convs, nhwc):
        """(route, sums, m) of layer i of the inference path on the activation h (a channels-last or plain tensor, or the
        `fftconv.GroupedMap` / `fftconv.LiftedInput` the previous layer left), decided from shapes alone: nothing is launched.
        route: "fft5" | "fftk" | "wino" | "lift_fused" | "lift_grouped" | "lift" | "lift_wide" | "lib", in this order of precedence.
        sums: the layer is the last before the tail and hands over the tail's window sums instead of its map.  m: Winograd's tile."""
        conv, tail = convs[i], convs[-1]
        cout, cin = bank.shape[:2]
        k, kt = conv.kernel_size, tail.kernel_size
        last_before_tail = i == len(convs) - 2
        if nhwc and self._plain_5x5(conv) and fftconv.applicable(h, cin, cout):
            # 5x5 regular->regular layer whose output the 44-pixel FFT tiles fit: overlap-save FFT convolution, 2.5 multiplies per
            # output (Winograd F(4x4,5x5): 4)
            return "fft5", (last_before_tail and kt in (3, 5) and tail.supports_linear_tail() and min(h.shape[-2:]) - 4 >= 2 * kt - 1), 0
        if (nhwc and not conv.lifting and k != 5 and conv.stride == 1 and conv.padding == 0
                and h.is_contiguous(memory_format=torch.channels_last) and fftconv.applicable_k(h.shape, cin, cout, k, h.device)):
            # regular -> regular layer of another kernel size (the reference's tutorial network: k = 9): the same overlap-save FFT
            # convolution with 49 - k outputs per tile (eqa_fft48_*); the linearised tail reads the map through the window-sum kernel
            return "fftk", False, 0
        if nhwc and self._plain_5x5(conv) and winograd.applicable(h, cin, cout):
            # 5x5 regular->regular layer: Winograd F(m x m, 5x5), m = 4 where the size allows -- or 2 where only that lets the output
            # transform emit the tail's window sums
            m = winograd.tile_for(h)
            if last_before_tail and not winograd.sums_applicable(h, kt, m) and winograd.sums_applicable(h, kt, 2):
                m = 2
            return "wino", last_before_tail and winograd.sums_applicable(h, kt, m), m
        lift = self._lift_kernel(conv, bank, h) if nhwc else None
        if lift == "narrow":
            # If the next layer is an FFT-convolved 5x5 layer, it computes each tile of this map from its input patch inside its own
            # forward transform (round 6: the layer does not run here at all); failing that the map goes out channel-group-major, the
            # layout that layer's input transform reads in whole cache lines (it is consumed by nothing else).
            nxt = convs[i + 1] if i + 1 < len(convs) - 1 else None
            if nxt is not None and self._plain_5x5(nxt):
                if fftconv.lift_fused_applicable(h.shape, bank.shape, nxt.out_channels * nxt.num_group_elements, h.device):
                    return "lift_fused", False, 0
                if fftconv.grouped_applicable((h.shape[0], cout, h.shape[2] - k + 1, h.shape[3] - k + 1), cout, cout, h.device):
                    return "lift_grouped", False, 0
            return "lift", False, 0
        return ("lift_wide" if lift == "wide" else "lib"), False, 0

    def _forward_inference(self, x: torch.Tensor) -> torch.Tensor:
        """eval + no_grad: conv(+folded BN) -> ReLU ... -> [last conv + group mean as window sums].  Per layer: `_route` decides,
        the loop body runs the route."""
        convs, norms = self._layers()
        tail = convs[-1]
        nhwc = (self.out_channels * self.num_group_elements) % 4 == 0
        h = x.contiguous(memory_format=torch.channels_last) if nhwc else x
        pending = None  # bias of the previous layer whose (bias + ReLU) has not been applied to `h` yet
        self.last_element, self.last_routes = None, []
        for i, (conv, bn) in enumerate(zip(convs[:-1], norms)):
            bank, bias = self._folded(conv, bn)
            route, sums, m = self._route(i, h, bank, convs, nhwc)
            self.last_routes.append(route)
            k, (H, W) = conv.kernel_size, h.shape[-2:]
            last_before_tail, shift = i == len(convs) - 2, None
            if route != "fft5" and isinstance(h, (fftconv.GroupedMap, fftconv.LiftedInput)):
                h = h.materialize()                 # written for an FFT layer that did not take it after all
            if route in ("fft5", "fftk", "wino"):
                # the previous layer's bias + ReLU ride on the input loads, this layer's on the way out; in front of the tail the output
                # transform emits the tail's window sums and the feature map is never written
                in_bias, pending = pending, None
                sums_k = tail.kernel_size if sums else 0
                if route == "wino":
                    U = self._cache.derived(conv, (conv, "wino", m), lambda: winograd.transform_filters(bank, m))
                    h = winograd.conv5x5(h, U, bias, relu=True, in_bias=in_bias, in_relu=in_bias is not None, sums_k=sums_k)
                else:
                    Bf = self._cache.derived(conv, (conv, "fft"), lambda: fftconv.spectra_for_k(bank))
                    if route == "fft5":
                        lifted = h if isinstance(h, fftconv.LiftedInput) else None
                        operands = sums_tail_operands(tail, bank.shape[0], H - k + 1, W - k + 1, self.element_tables) if sums else None
                        h = fftconv.conv5x5(h, Bf, bias, True, in_bias, in_bias is not None, sums_k=sums_k, tail=operands)
                        if lifted is not None and lifted.bound_route:
                            self.last_routes.append("bound:" + lifted.bound_route)
                        if operands is not None:
                            self.last_routes.append("tail:eqa_window_sums_tail")
                            self.last_element = h
                            return h[0]
                    else:
                        h = fftconv.conv_kxk(h, Bf, k, bias, True, in_bias, in_bias is not None)
            else:
                if pending is not None:  # this consumer cannot absorb it: apply in one fused pass
                    ops.bias_relu_nhwc_(h, pending)
                    pending = None
                if route == "lift_fused":
                    operand = {}
                    form = fftconv.LiftedInput.form_operand()     # the kernel form's packed filters, cached per weight version
                    if form is not None:
                        operand[form[1]] = self._cache.derived(conv, (conv, form[0]), lambda: form[2](bank))
                    h = fftconv.LiftedInput(h, bank, bias, True, **operand)
                elif route != "lib":                                  # the unfused lifting kernels: bias + ReLU in their epilogues
                    pack = ops.pack_lift_weights_wide if route == "lift_wide" else ops.pack_lift_weights
                    wpk = self._cache.derived(conv, (conv, "lift"), lambda: pack(bank))
                    if route == "lift_grouped":
                        h = fftconv.GroupedMap(ops.lift_conv_grouped(h, wpk, bias, True, k, k))
                    else:
                        h = (ops.lift_conv_wide if route == "lift_wide" else ops.lift_conv_nhwc)(h, wpk, bias, True, k, k)
                else:
                    h = F.conv2d(h, bank)
                    if last_before_tail:
                        shift = bias                                  # applied, with the ReLU, inside the tail's window-sum pass
                    elif nhwc and h.is_contiguous(memory_format=torch.channels_last):
                        pending = bias                                # deferred: fused into whatever reads h next
                    else:
                        h = torch.relu_(h + bias[None, :, None, None])
            if sums:
                self.last_routes.append("tail:finalize+eqa_window_sums_gemv")
                return window_sums_to_activations(h, tail, H - k + 1, W - k + 1)
            if last_before_tail:
                self.last_routes.append("tail:window_sums+eqa_window_sums_gemv")
                return conv_then_group_pool(h, tail, shift=shift, relu=shift is not None)
        raise AssertionError("unreachable: the network always has at least two convolutions")

    # -- training fast path ------------------------------------------------------------------------------------
    @staticmethod
    def _inner_bn(h: torch.Tensor, bn: nn.BatchNorm3d, E: int, conv_bias) -> torch.Tensor:
        """InnerBatchNorm on a channels-last (B, fields*E, H, W) map, op by op and differentiable by autograd (any device; the
        reference of the fused kernels' tests): statistics per field over (batch, group, space), fp64 accumulation, `_moments`."""
        Bn, C, H, W = h.shape
        Fd = C // E
        if bn.training or bn.running_mean is None:
            s1 = h.sum(dim=(0, 2, 3), dtype=torch.float64).view(Fd, E).sum(1)
            s2 = (h * h).sum(dim=(0, 2, 3), dtype=torch.float64).view(Fd, E).sum(1)
            mean, var = _moments(s1, s2, Bn * E * H * W, bn, conv_bias)
        else:
            mean = bn.running_mean if conv_bias is None else bn.running_mean - conv_bias
            var = bn.running_var
        scale = bn.weight * torch.rsqrt(var + bn.eps)
        shift = bn.bias - mean * scale
        return h * scale.repeat_interleave(E)[None, :, None, None] + shift.repeat_interleave(E)[None, :, None, None]

    def _train_route(self, li, h, bank, convs, bn):
        """(conv, with_stats, block) of hidden layer li of the training path on the channels-last activation h, decided from
        shapes and the EQA_TRAIN_* flags alone: nothing is launched.
        conv: "wino" | "fftk" | "lift" | "lift_wide" | "lib", in this order of precedence.  with_stats: the convolution takes the
        block's batch statistics in its epilogue.  block: "fused_tail" (the last hidden block goes straight into the window sums of
        the linearised final layer: its output is never written) | "fused" | "ops" (op by op, the reference of the fused kernels'
        tests; also what a library convolution that answers in another layout than channels-last gets)."""
        conv, kt = convs[li], convs[-1].kernel_size
        cout, cin = bank.shape[:2]
        k = conv.kernel_size
        fused = os.environ.get("EQA_TRAIN_FUSED_BN", "1") != "0"
        want_stats = (fused and os.environ.get("EQA_TRAIN_EPILOGUE_STATS", "1") != "0" and (bn.training or bn.running_mean is None))
        lift = self._lift_kernel(conv, bank, h, narrow_unchecked=True)
        with_stats = False
        if not conv.lifting and k == 5 and winograd.applicable(h, cin, cout):
            route, with_stats = "wino", want_stats and winograd.Conv5x5Function.stats_supported(h, bank)
        elif (not conv.lifting and k != 5
              and fftconv.applicable_k(h.shape, cin, cout, k, h.device, h.is_contiguous(memory_format=torch.channels_last))):
            route = "fftk"   # kernel sizes Winograd F(m, 5) does not cover (the tutorial's k = 9): forward and both gradients as FFT convolutions
        elif lift == "narrow":
            route, with_stats = "lift", want_stats and ops.lift_conv_stats_supported(h.shape, k, k, cout)
        else:
            route = "lift_wide" if lift == "wide" else "lib"
        OH, OW = h.shape[-2] - k + 1, h.shape[-1] - k + 1                     # (stride 1, no padding: `_training_fast_path_ok`)
        if (fused and li == len(convs) - 2 and os.environ.get("EQA_TRAIN_FUSED_TAIL", "1") != "0" and kt <= ops.MAX_WINDOW_K
                and OH > 2 * (kt - 1) and OW > 2 * (kt - 1) and h.shape[0] <= 65535):
            return route, with_stats, "fused_tail"
        return route, with_stats, "fused" if fused else "ops"

    def _forward_training(self, x: torch.Tensor) -> torch.Tensor:
        """Same layers as ``self.eqv_network`` + group pooling, with autograd, channels-last.  Per hidden layer `_train_route`
        decides, the loop body runs the decision: the convolution on the hand-written kernels with both gradients
        (``winograd.Conv5x5Function`` -- FFT or Winograd --, ``fftconv.ConvKxKFunction``, ``LiftConvFunction``) or the library's, then
        batch-norm / ReLU / dropout as one fused block (``InnerBnReluDropout``; the last one straight into the window sums:
        ``InnerBnReluDropoutWindowSums``) or op by op.  The last convolution + group mean are window sums + a GEMV."""
        convs, norms = self._layers()
        drops = [m for m in self.eqv_network if isinstance(m, nn.Dropout)]
        E = self.num_group_elements
        h = x.contiguous(memory_format=torch.channels_last)
        tail = convs[-1]
        S = None
        for li, (conv, bn, drop) in enumerate(zip(convs[:-1], norms, drops)):
            bank = conv.expanded_weights()
            route, with_stats, block = self._train_route(li, h, bank, convs, bn)
            if route == "wino":
                h = winograd.Conv5x5Function.apply(h, bank, winograd.tile_for(h), with_stats)
            elif route == "fftk":
                h = fftconv.ConvKxKFunction.apply(h, bank)
            elif route in ("lift", "lift_wide"):     # (wide: forward eqa_lift_conv_wide, filter gradient the framework's)
                h = LiftConvFunction.apply(h, bank, with_stats)
            else:
                h = F.conv2d(h, bank.contiguous(memory_format=torch.channels_last))
                if not h.is_contiguous(memory_format=torch.channels_last):
                    block = "ops"
            # part: the fp64 partial sums of the block's batch statistics, where the convolution kernel took them
            h, part = h if with_stats else (h, None)
            if block == "fused_tail":
                S = InnerBnReluDropoutWindowSums.apply(h, bn.weight, bn.bias, bn, E, conv.bias, drop.p, drop.training, tail.kernel_size, part)
            elif block == "fused":
                h = InnerBnReluDropout.apply(h, bn.weight, bn.bias, bn, E, conv.bias, drop.p, drop.training, part)
            else:
                h = F.dropout(torch.relu(self._inner_bn(h, bn, E, conv.bias)), drop.p, drop.training)
        k, O = tail.kernel_size, tail.out_channels
        H, W = h.shape[-2:]
        if S is None:
            S = WindowSumsFunction.apply(h, k)                                      # (B, C, k, k) fp64
        weff = tail.expanded_weights().view(O, E, -1).double().sum(0)               # (E, C*k*k), differentiable
        if S.is_cuda and S.dtype == torch.float64 and E <= 16 and os.environ.get("EQA_WS_TABLE_KERNEL", "1") != "0":
            act = WindowSumsLinearFn.apply(S.flatten(1), weff, 1.0 / float(O * (H - k + 1) * (W - k + 1)))     # (B, E) fp32
        else:
            act = S.flatten(1) @ weff.t() / float(O * (H - k + 1) * (W - k + 1))
        if tail.bias is not None:
            act = act + tail.bias.double().mean()
        # hidden-layer convolution biases cancel inside the batch-norms (zero gradient); keep them in the graph with that
        # exact zero so that DistributedDataParallel sees a gradient for every parameter
        hidden_bias = [c.bias.sum() for c in convs[:-1] if c.bias is not None]
        if hidden_bias:
            act = act + 0.0 * torch.stack(hidden_bias).sum().double()
        return act.float()

    def _training_fast_path_ok(self, x: torch.Tensor) -> bool:
        if self._dense or not x.is_cuda or x.dtype != torch.float32 or os.environ.get("EQA_TRAIN_FAST", "1") == "0":
            return False
        if (self.out_channels * self.num_group_elements) % 4 != 0:
            return False
        convs = [m for m in self.eqv_network if hasattr(m, "expanded_weights")]
        if len(convs) < 2 or any(c.stride != 1 or c.padding != 0 for c in convs) or not convs[-1].supports_linear_tail():
            return False
        hw = x.shape[-2] - (self.kernel_size - 1) * (len(convs) - 1)
        k = convs[-1].kernel_size
        return hw >= 2 * k - 1 and x.shape[-1] - (self.kernel_size - 1) * (len(convs) - 1) >= 2 * k - 1 and hw * hw <= 12288

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self.last_element = None
        if (self.training or torch.is_grad_enabled()) and self._training_fast_path_ok(x):
            return self._forward_training(x)
        if not self.training and not torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32:
            convs, norms = self._layers()
            shrink = (self.kernel_size - 1) * (len(convs) - 1)
            oh, ow = x.shape[-2] - shrink, x.shape[-1] - shrink
            # (the exported dense layers are not registered submodules, so .eval() does not reach them: a norm left in training
            # mode must take the module path with its batch statistics, not the folded running statistics)
            if (convs[-1].supports_linear_tail() and 0 < oh and 0 < ow and oh * ow <= 12288
                    and all(n.running_mean is not None and not n.training for n in norms)
                    and all(c.stride == 1 and c.padding == 0 and c.kernel_size == self.kernel_size for c in convs)):
                return self._forward_inference(x)
        if self._dense:
            convs, norms = self._dense
            for i, cv in enumerate(convs):
                x = cv(x)
                if i < len(norms):
                    x = F.relu(norms[i](x))
            fm = x.reshape(x.shape[0], self.out_channels, self.num_group_elements, x.shape[-2], x.shape[-1])
        else:
            fm = self.eqv_network(x)
        return group_pool(fm)


# (reference: same module; at the end because wrn_networks takes _InnerBatchNorm from this one)
from equiadapt_amd.images.canonicalization_networks.wrn_networks import (  # noqa: E402,F401
    ESCNNWideBasic,
    ESCNNWideBottleneck,
    ESCNNWRNEquivariantNetwork,
)
