"""ConvNetwork: the plain strided encoder the optimized canonicalizer scores group views with.

Reference: equiadapt/images/canonicalization_networks/custom_nonequivariant_networks.py:8-80.
Small MIOpen convolutions (PyTorch-ROCm); module / parameter names match the reference's state_dict.
The pretrained torchvision wrappers (ResNet18Network, WideResNet*) are out of scope.
"""
import os
import threading
from typing import List

import torch
from torch import nn

from equiadapt_amd.common.derived import DerivedCache, bn_eval_affine


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
