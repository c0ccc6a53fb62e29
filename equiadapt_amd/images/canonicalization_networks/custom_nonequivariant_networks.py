"""ConvNetwork: the plain strided encoder the optimized canonicalizer scores group views with; ResNet18Network: the ResNet-18 one;
WideResNet50Network / WideResNet101Network: the wide ResNets.

Reference: equiadapt/images/canonicalization_networks/custom_nonequivariant_networks.py:8-230.
Small MIOpen convolutions (PyTorch-ROCm); module / parameter names match the reference's state_dict.
ResNet18Network's eval forward runs 19 of its 20 convolutions on eqa_conv3x3_nhwc (csrc/conv3x3.hip); with EQA_RESNET_TRAIN_KERNEL=1
its training step runs them on that kernel, its two gradients and the eqa_bn_res_act_* block (csrc/conv3x3_train.hip).
The wide ResNets' eval forward runs every convolution behind the stem on eqa_convwide_nhwc (csrc/conv_wide.hip), which splits the K
loop over waves; their training is the plain modules.
"""
import os
import threading
from typing import List, Optional

import torch
from torch import nn

from equiadapt_amd.common.derived import DerivedCache, bn_eval_affine
from equiadapt_amd.common.utils import mark_written


_BN_FLAG_LOCK = threading.Lock()


class _ConvBnGeluFn(torch.autograd.Function):
    """One encoder layer in training, y = GELU(BatchNorm2d(conv_s2(x) + b)) with batch statistics, on the library's own kernels
    (reference: custom_nonequivariant_networks.py:44-57).  Forward: eqa_conv_s2 -> eqa_bn_stats_nhwc -> eqa_bn_act_fwd; backward:
    eqa_bn_act_bwd_reduce / _apply -> eqa_conv_s2_wgrad (+ eqa_conv_s2_dgrad for the layers behind the first).  x: the NCHW image
    batch for the first layer (planar), a (B,H,W,C) channels-last activation afterwards; y: (B,OH,OW,Cout) channels-last.  The
    convolution's bias gets an exactly zero gradient: behind a batch-norm with batch statistics the loss does not depend on it
    (autograd's own figure is the rounding noise of sum(dz))."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, bn, k, pad, planar):
        from equiadapt_amd import ops

        cout = w.shape[0]
        z = ops.conv_s2(x, ops.pack_conv_s2_weights(w.detach(), planar), None if b is None else b.detach(), False, cout, k, pad, planar)
        z2 = z.view(-1, cout)
        scale, shift, mean, rstd = ops.bn_fold_batch_stats(z2, bn)
        y = ops.bn_act_fwd(z2, scale, shift, None, 0).view(z.shape)
        ctx.save_for_backward(x, w, z, scale, shift, mean, rstd, gamma)
        ctx.geom = (k, pad, planar, b is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from equiadapt_amd import ops

        x, w, z, scale, shift, mean, rstd, gamma = ctx.saved_tensors
        k, pad, planar, has_bias = ctx.geom
        cout = w.shape[0]
        dz2, dgamma, dbeta = ops.bn_act_bwd(gy.contiguous().view(-1, cout), z.view(-1, cout), scale, shift, mean, rstd, gamma, None, 0)
        dz = dz2.view(z.shape)
        dw = ops.conv_s2_wgrad(x, dz, k, pad, planar) if ctx.needs_input_grad[1] else None
        db = torch.zeros(cout, dtype=w.dtype, device=w.device) if (has_bias and ctx.needs_input_grad[2]) else None
        dx = None
        if ctx.needs_input_grad[0]:
            if planar:
                raise RuntimeError("ConvNetwork: the image itself needs no gradient on the fused training path (EQA_CONVNET_TRAIN_MODE=cl_native)")
            dx = ops.conv_s2_dgrad(dz, ops.pack_conv_s2_dgrad_weights(w.detach()), (x.shape[1], x.shape[2]), x.shape[3], k, pad)
        return dx, dw, db, dgamma if ctx.needs_input_grad[3] else None, dbeta if ctx.needs_input_grad[4] else None, None, None, None, None


class _BnReluRowsFn(torch.autograd.Function):
    """The head's BatchNorm1d (batch statistics) -> Dropout1d -> ReLU on (rows, D) (custom_nonequivariant_networks.py:62-67):
    rowscale is Dropout1d's factor per ROW -- on a 2-D input the reference's Dropout1d drops whole samples (torch treats (N, D) as an
    unbatched (C, L) signal) -- or None; relu(r h) = r relu(h) for r >= 0, so the factor is applied behind the ReLU."""

    @staticmethod
    def forward(ctx, h, gamma, beta, bn, rowscale):
        from equiadapt_amd import ops

        scale, shift, mean, rstd = ops.bn_fold_batch_stats(h, bn)
        y = ops.bn_act_fwd(h, scale, shift, rowscale, 1)
        ctx.save_for_backward(h, scale, shift, mean, rstd, gamma, rowscale if rowscale is not None else torch.empty(0))
        ctx.has_rs = rowscale is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from equiadapt_amd import ops

        h, scale, shift, mean, rstd, gamma, rowscale = ctx.saved_tensors
        dh, dgamma, dbeta = ops.bn_act_bwd(gy.contiguous(), h, scale, shift, mean, rstd, gamma, rowscale if ctx.has_rs else None, 1)
        return dh if ctx.needs_input_grad[0] else None, dgamma, dbeta, None, None


class ConvNetwork(nn.Module):
    _mfma_chunk_override = None   # tests set this to run the inference fast path in small batch chunks

    def __init__(self, in_shape: tuple, out_channels: int, kernel_size: int, num_layers: int = 2,
                 out_vector_size: int = 128):
        super().__init__()
        chans = in_shape[0]
        blocks: List[nn.Module] = []
        for i in range(num_layers):
            widen = i > 0 and i % 3 == 2          # every third layer doubles the width (and pads by 1)
            nxt = 2 * out_channels if widen else out_channels
            blocks.append(nn.Conv2d(chans, nxt, kernel_size, 2, 1 if widen else 0))
            blocks += [nn.BatchNorm2d(nxt), nn.GELU()]
            chans = out_channels = nxt
        self.enc_network = nn.Sequential(*blocks)
        with torch.no_grad():
            was = self.enc_network.training
            probe = self.enc_network(torch.zeros(1, *in_shape)).shape   # same dry run as the reference ctor
            self.enc_network.train(was)
        out_dim = probe[1] * probe[2] * probe[3]
        self.final_fc = nn.Sequential(nn.BatchNorm1d(out_dim), nn.Dropout1d(0.5), nn.ReLU(),
                                      nn.Linear(out_dim, out_vector_size))
        self.out_vector_size = out_vector_size
        self._cache = DerivedCache()

    def _folded(self, conv: nn.Conv2d, bn: nn.BatchNorm2d):
        """Weights and bias of ``bn(conv(.))`` in eval mode (one convolution, no separate normalisation pass)."""
        def build():
            scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
            bias = conv.bias if conv.bias is not None else torch.zeros_like(scale)
            return (conv.weight * scale[:, None, None, None]).contiguous(), ((bias - bn.running_mean) * scale + bn.bias).contiguous()

        return self._cache.get(conv, (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var), build)

    def _plan_sources(self) -> list:
        """Every tensor `_mfma_plan` reads, straight from the modules' own tables: walking parameters() / buffers() costs ~20 us per
        forward, a tenth of a configs[4] step at B = 4."""
        mods = tuple(self.enc_network._modules.values())
        fc = self.final_fc._modules
        p, b = fc["0"]._parameters, fc["0"]._buffers
        src = [p["weight"], p["bias"], b["running_mean"], b["running_var"], fc["3"]._parameters["weight"]]
        for i in range(0, len(mods), 3):                           # (convolution, batch-norm, GELU)
            c, p, b = mods[i]._parameters, mods[i + 1]._parameters, mods[i + 1]._buffers
            src += (c["weight"], c["bias"], p["weight"], p["bias"], b["running_mean"], b["running_var"])
        return src

    def _mfma_plan(self, x: torch.Tensor):
        """Per layer (packed weights, bias, Cout, k, pad, planar) when EVERY convolution of the encoder fits eqa_conv_s2 (stride 2,
        k in {3,5,7}, first layer <= 4 input planes, then multiples of 16 channels), plus the head's parameters re-indexed from
        the reference's (C,H,W) flattening to the kernels' channels-last one; None otherwise."""
        return self._cache.get("mfma", self._plan_sources(), lambda: self._build_mfma_plan(x), x.shape[1:], x.device)

    def _build_mfma_plan(self, x: torch.Tensor):
        from equiadapt_amd import ops

        mods = list(self.enc_network)
        convs, bns = mods[0::3], mods[1::3]
        if any(not isinstance(a, nn.GELU) or a.approximate != "none" for a in mods[2::3]) or any(bn.running_mean is None for bn in bns):
            return None
        plan, layers, hw = None, [], tuple(x.shape[-2:])
        ok = True
        per_sample = [x.shape[1] * hw[0] * hw[1] * 4]      # bytes of every activation per sample (eqa_conv_s2 addresses < 2^31 bytes)
        for i, (conv, bn) in enumerate(zip(convs, bns)):
            k, pad = conv.kernel_size[0], conv.padding[0]
            if (conv.kernel_size[0] != conv.kernel_size[1] or conv.stride != (2, 2) or conv.padding[0] != conv.padding[1] or conv.groups != 1
                    or conv.dilation != (1, 1) or not ops.conv_s2_supported(conv.in_channels, conv.out_channels, k, pad, i == 0)):
                ok = False
                break
            w, b = self._folded(conv, bn)
            layers.append((ops.pack_conv_s2_weights(w, i == 0), b, conv.out_channels, k, pad, i == 0))
            hw = ((hw[0] + 2 * pad - k) // 2 + 1, (hw[1] + 2 * pad - k) // 2 + 1)
            per_sample.append(conv.out_channels * max(hw[0], 0) * max(hw[1], 0) * 4)
        bn1, lin = self.final_fc[0], self.final_fc[3]
        if ok and bn1.running_mean is not None and min(hw) > 0:
            C = convs[-1].out_channels
            # feature d of the reference = c * H * W + y * W + x; the kernels produce (y, x, c): gather the head's parameters
            idx = torch.arange(C * hw[0] * hw[1], device=x.device).view(C, hw[0], hw[1]).permute(1, 2, 0).reshape(-1)
            scale, shift = bn_eval_affine(bn1)
            # largest batch one eqa_conv_s2 call takes (every activation below 2^31 bytes); larger batches run in chunks, which
            # needs every per-sample activation to be a multiple of 16 bytes (the kernels' 16-byte loads start at the chunk's base)
            max_batch = (2 ** 31 - 64) // max(per_sample)
            chunkable = all(b % 16 == 0 for b in per_sample)
            plan = (layers, scale[idx].contiguous(), shift[idx].contiguous(), lin.weight[:, idx].contiguous(), max_batch, chunkable)
        return plan

    def _train_hip_applies(self, x: torch.Tensor) -> bool:
        """Training / autograd forward on the library's own kernels: every layer Conv2d(stride 2, k in 3/5/7, padding 0/1) over
        channel counts eqa_conv_s2 takes + affine BatchNorm2d + exact GELU, the module in training mode (batch statistics), fp32 on
        the device, the image needing no gradient, every activation below the kernels' 2 GiB addressing."""
        from equiadapt_amd import ops

        if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.shape[0] > 1 and not x.requires_grad and self.training):
            return False
        mods = list(self.enc_network)
        convs, bns, acts = mods[0::3], mods[1::3], mods[2::3]
        bn1 = self.final_fc[0]
        if any(not isinstance(a, nn.GELU) or a.approximate != "none" for a in acts) or not isinstance(bn1, nn.BatchNorm1d):
            return False
        if any(not bn.training or not bn.affine for bn in list(bns) + [bn1]) or bn1.num_features % 4:
            return False
        #  what the raw-pointer kernels assume and the module sequence does not: a dropout rate below 1 (rate 1 is 0 / 0
        # in the row mask; torch returns zeros), fp32 contiguous parameters and running statistics on x's device, no forward hooks on
        # the submodules the fused path would bypass.  Anything else takes the module sequence (cl_native).  Double backward
        # (gradient penalties, Hessian-vector products) also needs EQA_CONVNET_TRAIN_MODE=cl_native: the fused Functions are
        # once_differentiable.
        drop = self.final_fc[1]
        if not isinstance(drop, nn.Dropout1d) or not (0.0 <= drop.p < 1.0):
            return False
        lin = self.final_fc[3]
        for m in list(convs) + list(bns) + [bn1, lin]:
            for t in list(m._parameters.values()) + list(m._buffers.values()):
                if t is None or t.dtype == torch.int64:          # (num_batches_tracked)
                    continue
                if t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
                    return False
        if any(m._forward_hooks or m._forward_pre_hooks for m in list(self.enc_network.modules()) + list(self.final_fc.modules())):
            return False
        hw = tuple(x.shape[-2:])
        worst = x.shape[0] * x.shape[1] * hw[0] * hw[1] * 4
        for i, conv in enumerate(convs):
            k, pad = conv.kernel_size[0], conv.padding[0]
            if (conv.kernel_size[0] != conv.kernel_size[1] or conv.stride != (2, 2) or conv.padding[0] != conv.padding[1] or conv.groups != 1
                    or conv.dilation != (1, 1) or conv.padding_mode != "zeros" or hw[0] + 2 * pad < k or hw[1] + 2 * pad < k
                    or not ops.conv_s2_supported(conv.in_channels, conv.out_channels, k, pad, i == 0)
                    or not ops.conv_s2_train_supported(conv.in_channels, conv.out_channels, k, pad, i == 0)):
                return False
            hw = ((hw[0] + 2 * pad - k) // 2 + 1, (hw[1] + 2 * pad - k) // 2 + 1)
            worst = max(worst, x.shape[0] * conv.out_channels * hw[0] * hw[1] * 4)
        return worst < 2 ** 31 - 64 and min(hw) > 0

    def _forward_train_hip(self, x: torch.Tensor) -> torch.Tensor:
        mods = list(self.enc_network)
        h = x.contiguous()
        for i, (conv, bn) in enumerate(zip(mods[0::3], mods[1::3])):
            h = _ConvBnGeluFn.apply(h, conv.weight, conv.bias, bn.weight, bn.bias, bn, conv.kernel_size[0], conv.padding[0], i == 0)
        # the reference flattens (C, H, W); the kernels' activations are (H, W, C): one small copy (B x out_dim floats)
        h = h.permute(0, 3, 1, 2).reshape(h.shape[0], -1)
        bn1, drop, lin = self.final_fc[0], self.final_fc[1], self.final_fc[3]
        rowscale = None
        if drop.training and drop.p > 0:
            # Dropout1d on a 2-D input: torch reads (N, D) as an unbatched (C = N, L = D) signal and drops whole ROWS; the same
            # bernoulli_ / div_ sequence as at::feature_dropout on a (1, N, 1) noise tensor
            rowscale = torch.empty(1, h.shape[0], 1, dtype=h.dtype, device=h.device).bernoulli_(1 - drop.p).div_(1 - drop.p).view(-1)
        z = _BnReluRowsFn.apply(h, bn1.weight, bn1.bias, bn1, rowscale)
        return torch.nn.functional.linear(z, lin.weight, lin.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training and not torch.is_grad_enabled() and x.is_cuda:
            if x.dtype == torch.float32 and os.environ.get("EQA_CONVNET_MFMA", "1") != "0":
                plan = self._mfma_plan(x) if x.shape[0] > 0 else None     # (an empty batch takes the folded conv2d path below)
                if plan is not None and (x.shape[0] <= plan[4] or plan[5]) and plan[4] >= 1:
                    # inference: every convolution (+ folded batch-norm + GELU) on the fp32 matrix cores, channels-last from the
                    # first layer on; head = BatchNorm1d + ReLU in one pass + the Linear layer, re-indexed to that layout.
                    # (The optimised canonicalizer feeds G * B views at once: batches beyond the kernels' 2 GiB addressing run in
                    # chunks; shapes that can neither fit nor be chunked fall through to the folded conv2d path below.)
                    from equiadapt_amd import ops

                    layers, scale, shift, wlin, max_batch, chunkable = plan
                    if chunkable and self._mfma_chunk_override:       # tests: exercise the chunked form at a small size
                        max_batch = min(max_batch, int(self._mfma_chunk_override))
                    xc = x.contiguous()
                    outs = []
                    for lo in range(0, x.shape[0], max_batch):
                        h = xc[lo:lo + max_batch]
                        for wp, b, cout, k, pad, planar in layers:
                            h = ops.conv_s2(h, wp, b, True, cout, k, pad, planar)
                        outs.append(h.view(h.shape[0], -1))
                    z = ops.affine_relu_rows(outs[0] if len(outs) == 1 else torch.cat(outs), scale, shift)
                    return torch.nn.functional.linear(z, wlin, self.final_fc[3].bias)
            # inference: eval-mode batch-norms folded into the convolutions (three fewer passes over the feature maps)
            mods = list(self.enc_network)
            h = x
            for conv, bn, act in zip(mods[0::3], mods[1::3], mods[2::3]):
                if bn.running_mean is None:
                    h = act(bn(conv(h)))
                    continue
                w, b = self._folded(conv, bn)
                h = act(torch.nn.functional.conv2d(h, w, b, conv.stride, conv.padding, conv.dilation, conv.groups))
            h = h.reshape(x.shape[0], -1)
            bn1, lin = self.final_fc[0], self.final_fc[3]
            if h.dtype == torch.float32 and h.shape[1] % 4 == 0 and bn1.running_mean is not None:
                # head: BatchNorm1d (eval, folded) + [Dropout1d: identity] + ReLU in one pass, then the Linear layer
                from equiadapt_amd import ops

                scale, shift = self._cache.get("head", (bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var),
                                               lambda: tuple(t.contiguous() for t in bn_eval_affine(bn1)))
                return torch.nn.functional.linear(ops.affine_relu_rows(h.contiguous(), scale, shift), lin.weight, lin.bias)
            return self.final_fc(h)
        mode = os.environ.get("EQA_CONVNET_TRAIN_MODE", "hip")
        if mode == "hip" and self._train_hip_applies(x):
            return self._forward_train_hip(x)
        if mode == "hip":
            mode = "cl_native"
        if x.is_cuda and x.dim() == 4 and mode != "plain":
            # training (or autograd on): the reference's modules, run channels-last (MIOpen's fp32 convolutions are NHWC kernels)
            # with the batch-norms taken by ATen's channels-last kernels instead of MIOpen's.  Measured on the reference tutorial's
            # second loop (B = 512 x 4 views of 64 x 64, profiles/r04): as constructed (NCHW, MIOpen batch-norm: 0.4 TB/s,
            # 45 % of the step) 8.1 ms per step; channels-last with MIOpen's batch-norm 12.3; ATen's NCHW batch-norm 14.5;
            # channels-last + ATen's batch-norm 5.3 ms.  Same arithmetic and autograd formulas; the flattening in front of the
            # head follows the logical (C, H, W) order whatever the memory format.  EQA_CONVNET_TRAIN_MODE=plain: as constructed.
            h = x.contiguous(memory_format=torch.channels_last) if mode.startswith("cl") else x
            for m in self.enc_network:
                if isinstance(m, nn.BatchNorm2d) and mode.endswith("native"):
                    # ATen's channels-last batch-norm instead of MIOpen's: on ROCm only the process-global backend flag selects it (the
                    # op's own cudnn_enabled argument still lands in MIOpenBatchNorm*: measured, 41 k instead of 98 k img/s), so the
                    # toggle is taken under a lock -- interleaved save / restore from threaded replicas cannot leave the backend
                    # disabled for the process.  (Shapes eqa_conv_s2 takes do not come here: _forward_train_hip.)
                    with _BN_FLAG_LOCK, torch.backends.cudnn.flags(enabled=False):      # (the convolutions stay with MIOpen)
                        h = m(h)
                else:
                    h = m(h)
            return self.final_fc(h.reshape(x.shape[0], -1))
        return self.final_fc(self.enc_network(x).reshape(x.shape[0], -1))


class _BranchGrad:
    """The gradient of one branch of a basic block at the block's input, handed from the backward that makes it (the second
    batch-norm's residual, or the projection's data gradient) to the first convolution's data gradient, which adds it in its
    epilogue: the sum of the two branches costs no pass of its own.  The receiver's node depends on the giver's through the block, so
    the giver has always run; a hand-over that does not find its other end raises, it never drops a gradient."""

    def __init__(self):
        self.grad: Optional[torch.Tensor] = None

    def give(self, grad: torch.Tensor) -> None:
        if self.grad is not None:
            raise RuntimeError("ResNet18Network: a branch gradient was handed over twice before the block's first convolution took it")
        self.grad = grad

    def take(self) -> torch.Tensor:
        grad, self.grad = self.grad, None
        if grad is None:
            raise RuntimeError("ResNet18Network: the block's first convolution ran its backward before the other branch's gradient was there")
        return grad


class Conv3x3Function(torch.autograd.Function):
    """z = conv(x) of a basic block's 3 x 3 layer or 1 x 1 stride-2 shortcut on a (N, H, W, Cin) map (eqa_conv3x3_nhwc with a zero
    bias, no residual, no ReLU: in training the batch-norm behind it needs z itself), with its gradients, each only where it is
    needed: dW from eqa_conv3x3_wgrad, dx from eqa_conv3x3_dgrad -- or, with `wgrad_kernel` / `dgrad_kernel` false, the library's
    gradient on the same memory.  `take`: a _BranchGrad whose gradient is added to dx (in the kernel's epilogue); `give`: one that
    receives dx, autograd then being told that x has no gradient from here.  The caller has asked the three `ops.conv3x3*_supported`
    queries."""

    @staticmethod
    def forward(ctx, x, weight, taps, stride, zero_bias, wgrad_kernel=True, dgrad_kernel=True, take=None, give=None):
        from equiadapt_amd import ops

        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.geom = (taps, stride, wgrad_kernel, dgrad_kernel, take, give)
        return ops.conv3x3_nhwc(x, ops.pack_conv3x3_weights(weight.detach()), zero_bias, None, False, taps, stride)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        from equiadapt_amd import ops

        x, weight = ctx.saved_tensors
        taps, stride, wgrad_kernel, dgrad_kernel, take, give = ctx.geom
        dz = dz.contiguous()
        dx = dw = None
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        mask = (need_dx and not dgrad_kernel, need_dw and not wgrad_kernel, False)
        if mask[0] or mask[1]:
            pad = 1 if taps == 9 else 0
            dx, dw, _ = torch.ops.aten.convolution_backward(dz.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), weight, None, (stride, stride),
                                                            (pad, pad), (1, 1), False, (0, 0), 1, mask)
            if mask[0]:
                dx = dx.permute(0, 2, 3, 1)
                if take is not None:
                    dx = dx + take.take()
        if need_dw and wgrad_kernel:
            dw = ops.conv3x3_wgrad(x, dz, taps, stride)
        if need_dx and dgrad_kernel:
            dx = ops.conv3x3_dgrad(dz, ops.pack_conv3x3_dgrad_weights(weight.detach()), (x.shape[1], x.shape[2]),
                                   None if take is None else take.take(), taps, stride)
        if need_dx and give is not None:
            give.give(dx)
            dx = None
        return dx, dw, None, None, None, None, None, None, None


class BnResActFunction(torch.autograd.Function):
    """y = [relu](bn(z) [+ res]) with batch statistics on a (N, H, W, C) map -- the three forms of a basic block in training:
    relu(bn1(z)), relu(bn2(z) + shortcut), bn(z) on the projection -- on eqa_bn_act_stats / eqa_bn_act_finalize (which update the
    module's running statistics as nn.BatchNorm2d does) and eqa_bn_res_act_fwd; backward eqa_bn_res_act_bwd_reduce /
    eqa_bn_act_bwd_finalize / eqa_bn_res_act_bwd_apply -> gradients of z, gamma, beta and res.  `give`: a _BranchGrad that receives
    the residual's gradient instead of autograd."""

    @staticmethod
    def forward(ctx, z, gamma, beta, bn, res=None, relu=True, give=None):
        from equiadapt_amd import ops

        C = z.shape[-1]
        z = z.contiguous()
        z2 = z.view(-1, C)
        res2 = None if res is None else res.contiguous().view(-1, C)
        scale, shift, mean, rstd = ops.bn_fold_batch_stats(z2, bn)
        y = ops.bn_res_act_fwd(z2, scale, shift, res2, relu).view(z.shape)
        ctx.save_for_backward(z, scale, shift, mean, rstd, gamma, *(() if res is None else (res2,)))
        ctx.form = (relu, give)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        from equiadapt_amd import ops

        z, scale, shift, mean, rstd, gamma = ctx.saved_tensors[:6]
        res2 = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        relu, give = ctx.form
        C = z.shape[-1]
        need_dres = res2 is not None and (give is not None or ctx.needs_input_grad[4])
        dz, dgamma, dbeta, dres = ops.bn_res_act_bwd(gy.contiguous().view(-1, C), z.view(-1, C), scale, shift, mean, rstd, gamma.detach(), res2,
                                                     relu, need_dres)
        if dres is not None:
            dres = dres.view(z.shape)
            if give is not None:
                give.give(dres)
                dres = None
        return (dz.view(z.shape), dgamma if ctx.needs_input_grad[1] else None, dbeta if ctx.needs_input_grad[2] else None, None, dres, None,
                None)


class _BasicBlock(nn.Module):
    """The basic residual block of the published ResNet-18 (He et al. 2015, table 1, with the stride on the first 3 x 3 layer and a
    1 x 1 projection shortcut where the shape changes): relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x))."""

    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample: Optional[nn.Sequential] = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class _ResNet18(nn.Module):
    """ResNet-18 restated from its published definition, with the module names of torchvision's `resnet18` (so its state dict loads
    by key) and the reference's replacement head `fc = Sequential(Linear(512, out_vector_size))`."""

    def __init__(self, out_vector_size: int):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        widths = (64, 128, 256, 512)
        for i, wd in enumerate(widths):
            cin = widths[max(i - 1, 0)]
            setattr(self, f"layer{i + 1}", nn.Sequential(_BasicBlock(cin, wd, 1 if i == 0 else 2), _BasicBlock(wd, wd, 1)))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Sequential(nn.Linear(512, out_vector_size))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class ResNet18Network(nn.Module):
    """ResNet-18 with a `Linear(512, out_vector_size)` head as the canonicalization network (reference:
    custom_nonequivariant_networks.py:83-130; `network_type: non_equivariant_resnet18`).  As there, only `out_vector_size` of the
    constructor's arguments is used.  `self.resnet18` is a plain torch module with torchvision's parameter names, so a reference
    checkpoint loads by key.

    Weights: the reference downloads torchvision's ImageNet weights in its constructor; this package downloads nothing.  The network
    STARTS FROM RANDOM WEIGHTS (the published initialisation) unless a state dict is loaded -- a reference checkpoint through
    `load_state_dict`, or a torchvision `resnet18` state dict through `load_torchvision_state_dict`.

    Routes (`last_routes`: one string per convolution in module order, 20 entries):
      plain   `self.resnet18(x)`: any device, dtype, training mode, autograd.  `EQA_RESNET_KERNEL=0` (read per forward) forces it, and
              everything the fused rule does not take -- training in particular -- runs here.
      fused   the module and all its batch-norms in eval, gradients disabled, a 4-D fp32 input with 3 channels and B >= 1 on the device,
              parameters fp32, contiguous and on that device, no forward hooks on the submodules.  Every batch-norm is folded into the
              convolution in front of it; the stem is the library's convolution on a channels-last input ("lib") + relu_ + max_pool2d,
              used as a (B, h, w, 64) map without a copy; behind it every convolution is ONE launch of eqa_conv3x3_nhwc with bias
              (the folded norm), residual add and ReLU in its epilogue: a block's conv1 "conv3x3", its projection shortcut
              "conv1x1s2", its conv2 "conv3x3+res".  A layer `ops.conv3x3_supported` refuses, or one the gate `_kernel_pays` hands to
              the library (wide 3 x 3 layers at 2048 output pixels and more, where the library was measured faster), runs F.conv2d on
              the same channels-last memory + add_ + relu_ ("lib").  The tail is the mean over the pixels and F.linear.  No host
              synchronisation: the step can be captured into a hipGraph.
      train   opt-in, `EQA_RESNET_TRAIN_KERNEL=1` (read per forward; the default training route stays plain): the module and all its
              batch-norms in train(), affine and tracking running statistics, and the fused rule's conditions on input, parameters
              and hooks.  The stem runs through torch autograd on a channels-last input ("lib:train"); behind it every convolution
              is Conv3x3Function ("conv3x3:train", "conv1x1s2:train": eqa_conv3x3_nhwc forward, eqa_conv3x3_wgrad / eqa_conv3x3_dgrad
              backward, each gradient on the library instead where its gate on shapes says so: `last_wgrad_routes`) and every
              batch-norm BnResActFunction (batch statistics, the residual and the ReLU inside; running statistics updated as
              nn.BatchNorm2d does); a layer the queries refuse or `_kernel_pays` hands over runs F.conv2d under autograd
              ("lib:train").  The sum of the two branch gradients at a block's input rides in the first convolution's data gradient.
    """

    def __init__(self, in_shape: tuple, out_channels: int, kernel_size: int, num_layers: int = 2, out_vector_size: int = 128):
        super().__init__()
        self.resnet18 = _ResNet18(out_vector_size)
        self.out_vector_size = out_vector_size
        self.last_routes: List[str] = []
        self.last_wgrad_routes: List[str] = []     # per convolution, where its filter gradient runs on the training route: "kernel" / "lib"
        self._cache = DerivedCache()

    def load_torchvision_state_dict(self, state_dict) -> None:
        """Load the backbone from a torchvision `resnet18` state dict (keys without prefix), strictly; the dict's `fc.*` (1000 ImageNet
        classes, or any other width) is ignored and this network's head is left as it is."""
        sd = {k: v for k, v in state_dict.items() if not k.startswith("fc.")}
        sd.update({"fc." + k: v for k, v in self.resnet18.fc.state_dict().items()})
        self.resnet18.load_state_dict(sd, strict=True)

    def _blocks(self):
        net = self.resnet18
        return [b for layer in (net.layer1, net.layer2, net.layer3, net.layer4) for b in layer]

    def _pairs(self):
        """(convolution, batch-norm) in module order: the stem, then per block conv1, conv2 and the shortcut where there is one."""
        net = self.resnet18
        pairs = [(net.conv1, net.bn1)]
        for b in self._blocks():
            pairs += [(b.conv1, b.bn1), (b.conv2, b.bn2)]
            if b.downsample is not None:
                pairs.append((b.downsample[0], b.downsample[1]))
        return pairs

    def _fused_applies(self, x: torch.Tensor) -> bool:
        if self.training or torch.is_grad_enabled() or os.environ.get("EQA_RESNET_KERNEL", "1") == "0":
            return False
        return self._kernels_take(x, training=False)

    def _train_applies(self, x: torch.Tensor) -> bool:
        if not self.training or os.environ.get("EQA_RESNET_TRAIN_KERNEL", "0") != "1" or os.environ.get("EQA_RESNET_KERNEL", "1") == "0":
            return False
        return self._kernels_take(x, training=True)

    def _kernels_take(self, x: torch.Tensor, training: bool) -> bool:
        """What both kernel routes ask of the input, the parameters and the submodules; every batch-norm in the route's own mode."""
        if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and x.shape[0] >= 1):
            return False
        lin = self.resnet18.fc[0]
        for m in [m for pair in self._pairs() for m in pair] + [lin]:
            if isinstance(m, nn.BatchNorm2d) and (m.training != training or m.running_mean is None or not m.affine
                                                  or (training and not m.track_running_stats)):
                return False
            for t in list(m._parameters.values()) + list(m._buffers.values()):
                if t is None or t.dtype == torch.int64:          # (an absent bias; num_batches_tracked)
                    continue
                if t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
                    return False
        return not any(m._forward_hooks or m._forward_pre_hooks for m in self.resnet18.modules())

    def _folded(self, conv: nn.Conv2d, bn: nn.BatchNorm2d, pack: bool):
        """(filters, bias) of ``bn(conv(.))`` in eval mode -- the filters channels-last, as the library's convolution wants them beside a
        channels-last map -- and with `pack` the filters in eqa_conv3x3_nhwc's operand order: rebuilt when any tensor that enters them
        has changed (common/derived.py)."""
        def build():
            scale, shift = bn_eval_affine(bn)
            return (conv.weight * scale[:, None, None, None]).contiguous(memory_format=torch.channels_last), shift.contiguous()

        w, b = self._cache.get(conv, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), build)
        if not pack:
            return w, b
        from equiadapt_amd import ops

        return self._cache.derived(conv, (conv, "conv3x3"), lambda: ops.pack_conv3x3_weights(w)), b

    @staticmethod
    def _kernel_pays(pixels: int, cin: int, taps: int, stride: int) -> bool:
        """The gate on shapes alone (measured: DESIGN.md section 1, "ResNet18Network"): at 2048 output pixels and more, the library's
        convolution + add_ + relu_ is faster than the kernel on the 3 x 3 layers of 256 input channels and more, and on the stride-1
        ones of 128 and more.  Below 2048 pixels nothing was measured slower, and everything else stays on the kernel."""
        return not (taps == 9 and pixels >= 2048 and (cin >= 256 or (stride == 1 and cin >= 128)))

    def _layer(self, h: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, res: Optional[torch.Tensor], relu: bool, routes: list, slot: int):
        """One convolution + folded norm (+ residual) (+ ReLU) on the (B, h, w, C) map `h`: one launch where the kernel takes the shape
        and pays; else the library's convolution on the same memory (a channels-last view) with add_ and relu_ ("lib")."""
        from equiadapt_amd import ops

        taps, stride, pad = conv.kernel_size[0] ** 2, conv.stride[0], conv.padding[0]
        pixels = h.shape[0] * ((h.shape[1] + 2 * pad - conv.kernel_size[0]) // stride + 1) * ((h.shape[2] + 2 * pad - conv.kernel_size[0]) // stride + 1)
        if (ops.conv3x3_supported(h.shape[0], h.shape[1], h.shape[2], conv.in_channels, conv.out_channels, taps, stride)
                and self._kernel_pays(pixels, conv.in_channels, taps, stride)):
            wpk, b = self._folded(conv, bn, True)
            routes[slot] = "conv1x1s2" if taps == 1 else ("conv3x3" if res is None else "conv3x3+res")
            return ops.conv3x3_nhwc(h, wpk, b, res, relu, taps, stride)
        w, b = self._folded(conv, bn, False)
        routes[slot] = "lib"
        z = torch.nn.functional.conv2d(h.permute(0, 3, 1, 2), w, b, conv.stride, conv.padding)
        if res is not None:
            z.add_(res.permute(0, 3, 1, 2))
        if relu:
            z.relu_()
        z = z.permute(0, 2, 3, 1)
        return z if z.is_contiguous() else z.contiguous()

    def _forward_fused(self, x: torch.Tensor) -> torch.Tensor:
        net = self.resnet18
        routes = ["lib"] + [""] * 19
        w, b = self._folded(net.conv1, net.bn1, False)
        h = torch.nn.functional.conv2d(x.contiguous(memory_format=torch.channels_last), w, b, net.conv1.stride, net.conv1.padding)
        h = torch.nn.functional.max_pool2d(h.relu_(), 3, 2, 1).permute(0, 2, 3, 1)
        if not h.is_contiguous():
            h = h.contiguous()
        slot = 1
        for blk in self._blocks():
            t = self._layer(h, blk.conv1, blk.bn1, None, True, routes, slot)
            if blk.downsample is not None:
                h = self._layer(h, blk.downsample[0], blk.downsample[1], None, False, routes, slot + 2)
            h = self._layer(t, blk.conv2, blk.bn2, h, True, routes, slot + 1)
            slot += 2 if blk.downsample is None else 3
        self.last_routes = routes
        lin = net.fc[0]
        return torch.nn.functional.linear(h.mean(dim=(1, 2)), lin.weight, lin.bias)

    @staticmethod
    def _wgrad_pays(pixels: int, cin: int, cout: int, taps: int, stride: int) -> bool:
        """The filter gradient's own gate on shapes alone (measured: DESIGN.md section 1, "ResNet18Network", the training tables): at
        2304 output pixels and more the library's weight gradient was faster on all seven 3 x 3 forms and slower on the three 1 x 1
        shortcuts.  Below 2048 pixels nothing was measured, and the kernel keeps the layer."""
        return not (taps == 9 and pixels >= 2048)

    @staticmethod
    def _dgrad_pays(pixels: int, cin: int, cout: int, taps: int, stride: int) -> bool:
        """The data gradient's gate, likewise: at 2304 output pixels and more the library's was faster on all ten forms (at stride 2
        by 3 x: three taps in four are dropped loads whose matrix instructions still run)."""
        return pixels < 2048

    @staticmethod
    def _out_pixels(h: torch.Tensor, conv: nn.Conv2d) -> int:
        k, stride, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        return h.shape[0] * ((h.shape[1] + 2 * pad - k) // stride + 1) * ((h.shape[2] + 2 * pad - k) // stride + 1)

    def _train_kernel_takes(self, h: torch.Tensor, conv: nn.Conv2d) -> bool:
        from equiadapt_amd import ops

        k, stride = conv.kernel_size[0], conv.stride[0]
        shape = (h.shape[0], h.shape[1], h.shape[2], conv.in_channels, conv.out_channels, k * k, stride)
        return (ops.conv3x3_supported(*shape) and ops.conv3x3_dgrad_supported(*shape) and ops.conv3x3_wgrad_supported(*shape)
                and self._kernel_pays(self._out_pixels(h, conv), conv.in_channels, k * k, stride))

    def _train_layer(self, h, conv, bn, res, relu, slot, zero_bias, take=None, give=None, res_give=None):
        """One convolution + batch-norm with batch statistics (+ residual) (+ ReLU) on the (B, h, w, C) map `h` under autograd:
        Conv3x3Function where the kernels take the shape and pay, else the library's convolution on the same memory ("lib:train");
        BnResActFunction behind either."""
        taps, stride = conv.kernel_size[0] ** 2, conv.stride[0]
        if self._train_kernel_takes(h, conv):
            shape = (self._out_pixels(h, conv), conv.in_channels, conv.out_channels, taps, stride)
            wk, dk = self._wgrad_pays(*shape), self._dgrad_pays(*shape)
            self.last_routes[slot] = "conv1x1s2:train" if taps == 1 else "conv3x3:train"
            self.last_wgrad_routes[slot] = "kernel" if wk else "lib"
            z = Conv3x3Function.apply(h, conv.weight, taps, stride, zero_bias[:conv.out_channels], wk, dk, take, give)
        else:
            assert take is None and give is None
            self.last_routes[slot] = "lib:train"
            self.last_wgrad_routes[slot] = "lib"
            z = torch.nn.functional.conv2d(h.permute(0, 3, 1, 2), conv.weight, None, conv.stride, conv.padding).permute(0, 2, 3, 1)
        return BnResActFunction.apply(z, bn.weight, bn.bias, bn, res, relu, res_give)

    def _forward_train(self, x: torch.Tensor) -> torch.Tensor:
        net = self.resnet18
        self.last_routes = ["lib:train"] + [""] * 19
        self.last_wgrad_routes = ["lib"] + [""] * 19
        # The library's batch-norm writes its running statistics without moving their version counter, which the eval route's cache of
        # folded filters is keyed on (measured: the next fused forward ran on the stem's statistics from before the step).  The
        # counter moves BEFORE the call: the library keeps the two buffers for its backward, and autograd checks their version there.
        mark_written(net.bn1.running_mean, net.bn1.running_var)
        h = net.maxpool(net.relu(net.bn1(net.conv1(x.contiguous(memory_format=torch.channels_last))))).permute(0, 2, 3, 1)
        if not h.is_contiguous():
            h = h.contiguous()
        zero_bias = torch.zeros(512, dtype=torch.float32, device=x.device)
        slot = 1
        for blk in self._blocks():
            proj = blk.downsample
            # the shortcut's gradient at the block input rides in conv1's data gradient where both ends are kernels
            hint = None
            if h.requires_grad and self._train_kernel_takes(h, blk.conv1) and (proj is None or self._train_kernel_takes(h, proj[0])):
                hint = _BranchGrad()
            t = self._train_layer(h, blk.conv1, blk.bn1, None, True, slot, zero_bias, take=hint)
            if proj is not None:
                sc = self._train_layer(h, proj[0], proj[1], None, False, slot + 2, zero_bias, give=hint)
                h = self._train_layer(t, blk.conv2, blk.bn2, sc, True, slot + 1, zero_bias)
            else:
                h = self._train_layer(t, blk.conv2, blk.bn2, h, True, slot + 1, zero_bias, res_give=hint)
            slot += 2 if proj is None else 3
        lin = net.fc[0]
        return torch.nn.functional.linear(h.mean(dim=(1, 2)), lin.weight, lin.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fused_applies(x):
            return self._forward_fused(x)
        self.last_wgrad_routes = []
        if self._train_applies(x):
            return self._forward_train(x)
        self.last_routes = ["plain"] * 20
        return self.resnet18(x)


class _Bottleneck(nn.Module):
    """The bottleneck residual block of the published wide ResNet (He et al. 2015, table 1, with the inner width doubled as in
    Zagoruyko & Komodakis 2016 and torchvision's `wide_resnet*_2`; the stride on the 3 x 3 layer): 1 x 1 to 2 planes, 3 x 3, 1 x 1 to
    4 planes, relu(bn3(conv3(.)) + shortcut(x)) with a 1 x 1 projection shortcut in the first block of every layer."""

    def __init__(self, cin: int, planes: int, stride: int, project: bool):
        super().__init__()
        width = 2 * planes
        self.conv1 = nn.Conv2d(cin, width, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, 4 * planes, 1, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample: Optional[nn.Sequential] = None
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * planes, 1, stride, bias=False), nn.BatchNorm2d(4 * planes))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class _WideResNet(nn.Module):
    """The wide ResNet-50-2 / ResNet-101-2 restated from the published definition, with the module names of torchvision's
    `wide_resnet50_2` / `wide_resnet101_2` (so their state dicts load by key) and the reference's replacement head
    `fc = Sequential(Linear(2048, out_vector_size))`."""

    def __init__(self, blocks: tuple, out_vector_size: int):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for i, (planes, count) in enumerate(zip((64, 128, 256, 512), blocks)):
            layer = [_Bottleneck(cin, planes, 1 if i == 0 else 2, True)]
            cin = 4 * planes
            layer += [_Bottleneck(cin, planes, 1, False) for _ in range(count - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*layer))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Sequential(nn.Linear(2048, out_vector_size))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class _WideResNetNetwork(nn.Module):
    """A wide ResNet with a `Linear(2048, out_vector_size)` head as the canonicalization network (reference:
    custom_nonequivariant_networks.py:133-230; `network_type: non_equivariant_wrn_50` / `non_equivariant_wrn_101`).  As there, only
    `out_vector_size` of the constructor's arguments is used.  `self.wideresnet` is a plain torch module with torchvision's parameter
    names, so a reference checkpoint loads by key.

    Weights: the reference downloads torchvision's ImageNet weights in its constructor; this package downloads nothing.  The network
    STARTS FROM RANDOM WEIGHTS (the published initialisation) unless a state dict is loaded -- a reference checkpoint through
    `load_state_dict`, or a torchvision `wide_resnet50_2` / `wide_resnet101_2` state dict through `load_torchvision_state_dict`.

    Routes (`last_routes`: one string per convolution in module order -- the stem, then per block conv1, conv2, conv3 and
    downsample.0 where present: 53 / 104 entries; `last_ksplits`: the K slices of each kernel call, 0 for "lib", the stem and plain):
      plain   `self.wideresnet(x)`: any device, dtype, training mode, autograd.  `EQA_WIDERESNET_KERNEL=0` (read per forward) forces
              it, and everything the fused rule does not take -- training in particular -- runs here.
      fused   ResNet18Network's rule: the module and all its batch-norms in eval, gradients disabled, a 4-D fp32 input with 3 channels
              and B >= 1 on the device, parameters fp32, contiguous and on that device, no forward hooks on the submodules.  Every
              batch-norm is folded into the convolution in front of it; the stem is the library's convolution on a channels-last
              input ("lib") + relu_ + max_pool2d, used as a (B, h, w, 64) map without a copy; behind it every convolution is one call
              of eqa_convwide_nhwc (csrc/conv_wide.hip) with bias (the folded norm), residual add and ReLU inside: a block's conv1
              "conv1x1", conv2 "conv3x3", projection "proj", conv3 "conv1x1+res".  A layer `ops.convwide_supported` refuses, or one the
              gate `_kernel_pays` hands to the library, runs F.conv2d on the same channels-last memory + add_ + relu_ ("lib").  The
              tail is the mean over the pixels and F.linear.  No host synchronisation: the step can be captured into a hipGraph.
    """

    _BLOCKS: tuple = ()

    def __init__(self, in_shape: tuple, out_channels: int, kernel_size: int, num_layers: int = 2, out_vector_size: int = 128):
        super().__init__()
        self.wideresnet = _WideResNet(self._BLOCKS, out_vector_size)
        self.out_vector_size = out_vector_size
        self.last_routes: List[str] = []
        self.last_ksplits: List[int] = []
        self._cache = DerivedCache()

    def load_torchvision_state_dict(self, state_dict) -> None:
        """Load the backbone from a torchvision `wide_resnet50_2` / `wide_resnet101_2` state dict (keys without prefix), strictly; the
        dict's `fc.*` (1000 ImageNet classes, or any other width) is ignored and this network's head is left as it is."""
        sd = {k: v for k, v in state_dict.items() if not k.startswith("fc.")}
        sd.update({"fc." + k: v for k, v in self.wideresnet.fc.state_dict().items()})
        self.wideresnet.load_state_dict(sd, strict=True)

    def _blocks(self):
        net = self.wideresnet
        return [b for layer in (net.layer1, net.layer2, net.layer3, net.layer4) for b in layer]

    def _pairs(self):
        """(convolution, batch-norm) in module order: the stem, then per block conv1, conv2, conv3 and the shortcut where there is one."""
        net = self.wideresnet
        pairs = [(net.conv1, net.bn1)]
        for b in self._blocks():
            pairs += [(b.conv1, b.bn1), (b.conv2, b.bn2), (b.conv3, b.bn3)]
            if b.downsample is not None:
                pairs.append((b.downsample[0], b.downsample[1]))
        return pairs

    def _fused_applies(self, x: torch.Tensor) -> bool:
        if self.training or torch.is_grad_enabled() or os.environ.get("EQA_WIDERESNET_KERNEL", "1") == "0":
            return False
        if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and x.shape[0] >= 1):
            return False
        lin = self.wideresnet.fc[0]
        for m in [m for pair in self._pairs() for m in pair] + [lin]:
            if isinstance(m, nn.BatchNorm2d) and (m.training or m.running_mean is None or not m.affine):
                return False
            for t in list(m._parameters.values()) + list(m._buffers.values()):
                if t is None or t.dtype == torch.int64:          # (an absent bias; num_batches_tracked)
                    continue
                if t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
                    return False
        return not any(m._forward_hooks or m._forward_pre_hooks for m in self.wideresnet.modules())

    def _folded(self, conv: nn.Conv2d, bn: nn.BatchNorm2d, pack: bool):
        """(filters, bias) of ``bn(conv(.))`` in eval mode -- the filters channels-last, as the library's convolution wants them beside a
        channels-last map -- and with `pack` the filters in eqa_convwide_nhwc's operand order (eqa_conv3x3_nhwc's): rebuilt when any
        tensor that enters them has changed (common/derived.py)."""
        def build():
            scale, shift = bn_eval_affine(bn)
            return (conv.weight * scale[:, None, None, None]).contiguous(memory_format=torch.channels_last), shift.contiguous()

        w, b = self._cache.get(conv, (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var), build)
        if not pack:
            return w, b
        from equiadapt_amd import ops

        return self._cache.derived(conv, (conv, "convwide"), lambda: ops.pack_conv3x3_weights(w)), b

    @staticmethod
    def _kernel_pays(pixels: int, cin: int, cout: int, taps: int, stride: int) -> bool:
        """The gate on shapes alone (measured: DESIGN.md section 1, "WideResNet50Network / WideResNet101Network"): the forms measured
        slower than the library's convolution + add_ + relu_ by more than the spread between rounds go to the library from the pixel
        count at which they were measured -- the 3 x 3 layers of 256 input channels from 36864 output pixels, of 512 from 9216, of
        1024 from 2304, and the 1 x 1 layers with 2048 channels on either side from 2304.  Everything else, and everything smaller,
        stays on the kernel: nothing was measured slower there."""
        if taps == 9:
            floor = {256: 36864, 512: 9216, 1024: 2304}.get(cin)
            return floor is None or pixels < floor
        return not (max(cin, cout) == 2048 and pixels >= 2304)

    def _layer(self, h: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, res: Optional[torch.Tensor], relu: bool, route: str, slot: int):
        """One convolution + folded norm (+ residual) (+ ReLU) on the (B, h, w, C) map `h`: one call of the kernel where it takes the
        shape and pays; else the library's convolution on the same memory (a channels-last view) with add_ and relu_ ("lib")."""
        from equiadapt_amd import ops

        k, stride, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        shape = (h.shape[0], h.shape[1], h.shape[2], conv.in_channels, conv.out_channels, k * k, stride)
        pixels = h.shape[0] * ((h.shape[1] + 2 * pad - k) // stride + 1) * ((h.shape[2] + 2 * pad - k) // stride + 1)
        if ops.convwide_supported(*shape) and self._kernel_pays(pixels, conv.in_channels, conv.out_channels, k * k, stride):
            wpk, b = self._folded(conv, bn, True)
            ksplit = ops.convwide_ksplit(*shape)
            self.last_routes[slot], self.last_ksplits[slot] = route, ksplit
            return ops.convwide_nhwc(h, wpk, b, res, relu, k * k, stride, ksplit)
        w, b = self._folded(conv, bn, False)
        self.last_routes[slot], self.last_ksplits[slot] = "lib", 0
        z = torch.nn.functional.conv2d(h.permute(0, 3, 1, 2), w, b, conv.stride, conv.padding)
        if res is not None:
            z.add_(res.permute(0, 3, 1, 2))
        if relu:
            z.relu_()
        z = z.permute(0, 2, 3, 1)
        return z if z.is_contiguous() else z.contiguous()

    def _forward_fused(self, x: torch.Tensor) -> torch.Tensor:
        net = self.wideresnet
        n = len(self._pairs())
        self.last_routes, self.last_ksplits = ["lib"] + [""] * (n - 1), [0] * n
        w, b = self._folded(net.conv1, net.bn1, False)
        h = torch.nn.functional.conv2d(x.contiguous(memory_format=torch.channels_last), w, b, net.conv1.stride, net.conv1.padding)
        h = torch.nn.functional.max_pool2d(h.relu_(), 3, 2, 1).permute(0, 2, 3, 1)
        if not h.is_contiguous():
            h = h.contiguous()
        slot = 1
        for blk in self._blocks():
            t = self._layer(h, blk.conv1, blk.bn1, None, True, "conv1x1", slot)
            t = self._layer(t, blk.conv2, blk.bn2, None, True, "conv3x3", slot + 1)
            if blk.downsample is not None:
                h = self._layer(h, blk.downsample[0], blk.downsample[1], None, False, "proj", slot + 3)
            h = self._layer(t, blk.conv3, blk.bn3, h, True, "conv1x1+res", slot + 2)
            slot += 3 if blk.downsample is None else 4
        lin = net.fc[0]
        return torch.nn.functional.linear(h.mean(dim=(1, 2)), lin.weight, lin.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fused_applies(x):
            return self._forward_fused(x)
        n = len(self._pairs())
        self.last_routes, self.last_ksplits = ["plain"] * n, [0] * n
        return self.wideresnet(x)


class WideResNet50Network(_WideResNetNetwork):
    __doc__ = "Wide ResNet-50-2 (bottleneck blocks 3, 4, 6, 3; 53 convolutions).  " + _WideResNetNetwork.__doc__
    _BLOCKS = (3, 4, 6, 3)


class WideResNet101Network(_WideResNetNetwork):
    __doc__ = "Wide ResNet-101-2 (bottleneck blocks 3, 4, 23, 3; 104 convolutions).  " + _WideResNetNetwork.__doc__
    _BLOCKS = (3, 4, 23, 3)
