"""Group pooling: (B, C, G, H', W') -> (B, G) activations on the HIP streaming-reduction kernel."""
import os

import torch

from equiadapt_amd import _lib, ops


class _GroupPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feature_map: torch.Tensor) -> torch.Tensor:
        ctx.shape = tuple(feature_map.shape)
        act, _ = ops.group_pool_argmax(feature_map, want_index=False)
        return act

    @staticmethod
    def backward(ctx, grad_act: torch.Tensor):
        B, C, G, H, W = ctx.shape
        # d mean / d feature = 1 / (C*H*W), broadcast: left to autograd consumers as an expanded view
        return (grad_act / float(C * H * W))[:, None, :, None, None].expand(B, C, G, H, W)


def group_pool(feature_map: torch.Tensor) -> torch.Tensor:
    """``torch.mean(feature_map, dim=(1, 3, 4))`` (reference: escnn_networks.py:115,
    custom_equivariant_networks.py:91) as one pass over the map (eqa_group_pool_argmax; fp32 -- a module converted to
    another dtype, e.g. ``.double()`` for a reference computation, takes torch's reduction)."""
    if feature_map.dtype != torch.float32:
        return torch.mean(feature_map, dim=(1, 3, 4))
    return _GroupPoolFn.apply(feature_map)


def conv_then_group_pool(h: torch.Tensor, layer, scale=None, shift=None, relu: bool = False) -> torch.Tensor:
    """``group_pool(layer(act(h)))`` WITHOUT running the convolution (inference fast path; exact up to fp rounding).

    The mean over (fields, space) of a convolution is linear in its input, so
        act[b, g] = sum_{c,u,v} Weff[g,c,u,v] * S[b,c,u,v] / count + mean(bias),
    with Weff = the filter bank summed over output fields and S the k*k shifted-window sums of each input plane
    (``eqa_window_sums``, one pass over ``h``; ``act(t) = [relu](scale*t + shift)`` per channel folds the previous
    layer's bias / eval-mode batch-norm / ReLU into that pass).  ``layer`` is a group conv with stride 1, padding 0.
    """
    k, E, O = layer.kernel_size, layer.num_group_elements, layer.out_channels
    B, _, H, W = h.shape
    S = ops.window_sums(h, k, scale, shift, relu)                       # (B, Cin, k, k) fp64
    return window_sums_to_activations(S, layer, H, W)


def window_sums_to_activations(S: torch.Tensor, layer, H: int, W: int) -> torch.Tensor:
    """The GEMV half of ``conv_then_group_pool``: (B, Cin, k, k) fp64 window sums of the (H, W) input -> (B, G)."""
    k, O = layer.kernel_size, layer.out_channels
    weff = layer.mean_response_weights()                                # (E, Cin*k*k) fp64
    scale = 1.0 / float(O * (H - k + 1) * (W - k + 1))
    if S.is_cuda and weff.shape[0] <= 16 and not torch.is_grad_enabled():
        return ops.window_sums_gemv(S.flatten(1), weff, scale, layer.mean_bias_value())
    act = S.flatten(1) @ weff.t() * scale
    if layer.bias is not None:
        mb = layer.mean_bias_value()                                    # a float, or one value per element (exported dense form)
        act = act + (mb if isinstance(mb, float) else mb.to(act.device))
    return act.float()


def sums_tail_operands(layer, cin: int, H: int, W: int, tables):
    """The operands of ``ops.window_sums_tail`` for `layer` on an (H, W) map of `cin` channels and the canonicalizer's element
    `tables` (rotation, reflection or None; fp32, one entry per group element), or None where that launch does not apply and the
    tail runs as `window_sums_to_activations` and the canonicalizer's own lookups (``EQA_TAIL_FUSED=0`` forces that)."""
    if tables is None or os.environ.get("EQA_TAIL_FUSED", "1") == "0" or torch.is_grad_enabled():
        return None
    k, O = layer.kernel_size, layer.out_channels
    weff, shift = layer.mean_response_weights(), layer.mean_bias_value()
    E = weff.shape[0]
    rot, ref = tables
    if not (isinstance(shift, float) and weff.is_cuda and ops.window_sums_tail_supported(cin, k, E)):
        return None
    if any(t is not None and (t.dtype != torch.float32 or t.device != weff.device or t.numel() != E or not t.is_contiguous()) for t in (rot, ref)):
        return None
    return weff, 1.0 / float(O * (H - k + 1) * (W - k + 1)), shift, rot, ref


class WindowSumsLinearFn(torch.autograd.Function):
    """act = scale * S . weff^T, the GEMV of the linearised last layer, with its backward (dS = scale * dact . weff,
    dweff = scale * dact^T . S) on the library's kernels: eqa_window_sums_gemv / eqa_window_sums_gemv_bwd.  S:(B,K) fp64,
    weff:(E <= 16, K) fp64 -> (B,E) fp32.  (Through torch these are three fp64 library GEMMs with an inner or outer dimension of 4-8.)"""

    @staticmethod
    def forward(ctx, S, weff, scale):
        S, weff = S.contiguous(), weff.contiguous()
        ctx.save_for_backward(S, weff)
        ctx.scale = scale
        return ops.window_sums_gemv(S, weff, scale, 0.0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dact):
        S, weff = ctx.saved_tensors
        dS, dW = ops.window_sums_gemv_bwd(dact.float().contiguous(), weff, S, ctx.scale, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dS, dW, None


def window_grad_table(dS: torch.Tensor, H: int, W: int, k: int) -> torch.Tensor:
    """Backward of the k*k shifted-window sums of an (H, W) map as a table: a pixel's gradient depends only on the class of its row and
    of its column (the k-1 top / left border indices, the interior, the k-1 bottom / right ones): (B, C, k, k) -> (B, 2k-1, 2k-1, C) fp32.
    On eqa_window_grad_table where it applies, else (and under EQA_WS_TABLE_KERNEL=0) as an fp64 mask einsum."""
    nb, dev = k - 1, dS.device
    if (dS.is_cuda and dS.dtype == torch.float64 and k <= ops.MAX_WINDOW_K and dS.shape[0] <= 65535 and H >= 2 * nb + 1 and W >= 2 * nb + 1
            and os.environ.get("EQA_WS_TABLE_KERNEL", "1") != "0"):
        return ops.window_grad_table(dS.contiguous(), H, W)       # rectangle sums from prefix sums: one launch, no library GEMM

    def mask(n):
        rep = torch.cat([torch.arange(nb), torch.tensor([nb]), torch.arange(n - nb, n)]).to(dev)       # one representative per class
        u = torch.arange(k, device=dev)
        return ((u[None, :] <= rep[:, None]) & (rep[:, None] <= u[None, :] + (n - k))).to(dS.dtype)    # (2nb+1, k)

    return torch.einsum("tu,bcuv,sv->btsc", mask(H), dS, mask(W)).float().contiguous()


class WindowSumsFunction(torch.autograd.Function):
    """S[b,c,u,v] = sum over the (H-k+1, W-k+1) window at (u, v) of x[b,c] (fp64), with its backward: a pixel (y, x) receives
    the sum of dS over the windows that contain it.  Rows fall into 2(k-1)+1 classes (the k-1 top rows, the interior, the k-1
    bottom rows), columns likewise, so the gradient is a (2k-1) x (2k-1) table per (b, c), expanded to the map by `eqa_window_sums_bwd_expand_nhwc`.
    Training counterpart of `conv_then_group_pool` (the last convolution + group mean are linear in x)."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k, ctx.shape = k, x.shape
        ctx.channels_last = x.is_contiguous(memory_format=torch.channels_last)
        return ops.window_sums(x, k)

    @staticmethod
    def backward(ctx, dS):
        k = ctx.k
        B, C, H, W = ctx.shape
        table = window_grad_table(dS, H, W, k)                                   # (B, 2k-1, 2k-1, C), channels last
        if table.is_cuda and C % 4 == 0:
            g = torch.empty((B, H, W, C), dtype=torch.float32, device=table.device)
            with torch.cuda.device(table.device):
                st = _lib.load().eqa_window_sums_bwd_expand_nhwc(table.data_ptr(), g.data_ptr(), B, H, W, C, k, ops._stream())
            _lib.check(st, "eqa_window_sums_bwd_expand_nhwc")
        else:
            def cls(n):                                                          # class of each of n rows / columns
                i = torch.arange(n, device=table.device)
                return torch.where(i < k - 1, i, torch.where(i >= n - (k - 1), i - (n - (k - 1)) + k, torch.full_like(i, k - 1)))

            g = table[:, cls(H)][:, :, cls(W)]                                   # (B, H, W, C)
        g = g.permute(0, 3, 1, 2)                                                # NCHW view of channels-last memory
        if not ctx.channels_last:
            g = g.contiguous()
        return g, None
