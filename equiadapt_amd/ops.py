"""Tensor-level entry points over the C ABI (include/eqa_hip.h).

Every function takes ROCm ("cuda") fp32 tensors, launches on torch's current HIP stream and returns
torch tensors; nothing here computes on the CPU.  torch is plumbing only: device memory + streams.
"""
import os
from typing import Optional, Tuple

import torch

from equiadapt_amd import _lib
from equiadapt_amd.common.derived import _stamp


MAX_WINDOW_K = 10   # == kMaxWinK (csrc/eqa_common.hpp): the largest window the window-sum kernels take (the linearised last layer)
VNSMALL_PARAMS = 1310       # == EQA_VNSMALL_PARAMS (include/eqa_hip.h): packed VNSmall parameters, pooling "mean" (layout: csrc/vn_common.hpp)
VNSMALL_PARAMS_MAX = 1751   # == EQA_VNSMALL_PARAMS_MAX: pooling "max", + the pooling layer's 21 x 21 direction map


def _stream() -> int:
    """The raw handle of torch's current HIP stream on the current device.  (torch.cuda.current_stream() builds a Stream object
    through four Python frames: 4-9 us per call, twelve calls in a configs[4] step -- a fifth of its host time at B = 4.)"""
    return _raw_stream(_current_device())


try:                                   # private but stable since torch 1.x (inductor's own launcher uses the first)
    _raw_stream, _current_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
except AttributeError:                 # a torch without them: the public, slower spelling
    def _raw_stream(_dev):
        return torch.cuda.current_stream().cuda_stream

    def _current_device():
        return 0


class KernelTimer:
    """HIP-event bracket around named launches, recorded on the stream the kernels run on.

    ``with ops.KernelTimer() as t: ...`` then ``t.summary()`` -> {name: (launches, mean_ms)} after a
    device synchronise.  Used by bench.py for the live per-kernel duration behind ``roofline.achieved``.
    """

    active: "Optional[KernelTimer]" = None

    def __init__(self):
        self.events = {}

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.events.items()}


class _timed:
    def __init__(self, name: str):
        self.t = KernelTimer.active
        self.name = name

    def __enter__(self):
        if self.t is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.t is not None:
            self.b.record()
            self.t.events.setdefault(self.name, []).append((self.a, self.b))


def _need(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: equiadapt_amd runs on an MI355X (ROCm) device only, no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype} (the hot path computes in fp32 like the reference)")
    return t if t.is_contiguous() else t.contiguous()


def _opt(t: Optional[torch.Tensor], name: str, dtype) -> Tuple[Optional[torch.Tensor], Optional[int]]:
    if t is None:
        return None, None
    t = _need(t, name, dtype)
    return t, t.data_ptr()


def group_action(
    src: torch.Tensor,
    gidx: Optional[torch.Tensor],
    theta: torch.Tensor,
    flags: Optional[torch.Tensor],
    chan_map: Optional[torch.Tensor],
    pad: int,
    out_hw: Tuple[int, int],
    top_left: Tuple[int, int],
    n_out: Optional[int] = None,
) -> torch.Tensor:
    """Generic discrete group action on image planes (eqa_group_action_fwd)."""
    lib = _lib.load()
    src = _need(src, "src")
    theta = _need(theta, "theta")
    B, C, H, W = src.shape
    E = theta.shape[0]
    gidx, p_gidx = _opt(gidx, "gidx", torch.int32)
    flags, p_flags = _opt(flags, "flags", torch.int32)
    chan_map, p_map = _opt(chan_map, "chan_map", torch.int32)
    G = chan_map.shape[1] if chan_map is not None else 1
    if n_out is None:
        n_out = B if gidx is not None else E * B
    OH, OW = out_hw
    dst = torch.empty((n_out, C, OH, OW), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        st = lib.eqa_group_action_fwd(src.data_ptr(), dst.data_ptr(), p_gidx, theta.data_ptr(), p_flags, p_map, E, G,
                                      n_out, B, C, H, W, pad, OH, OW, top_left[0], top_left[1], _stream())
    _lib.check(st, "eqa_group_action_fwd")
    return dst


def group_action_bwd(
    src: torch.Tensor,
    grad_out: torch.Tensor,
    gidx: Optional[torch.Tensor],
    theta: torch.Tensor,
    flags: Optional[torch.Tensor],
    chan_map: Optional[torch.Tensor],
    pad: int,
    top_left: Tuple[int, int],
    want_src: bool,
    want_angle: bool,
    want_theta: bool = False,
) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Backward of ``group_action`` (eqa_group_action_bwd / eqa_group_action_bwd_theta).

    Returns (dL/d src or None, dL/d angle or None); the angle gradient is per output image and w.r.t. the
    ``angle`` argument IN DEGREES of the ``rotate(img, angle)`` that ``theta`` encodes.  With ``want_theta`` the second
    value is instead dL/d theta, (n_out, 6), for a per-output affine matrix (continuous groups).
    """
    lib = _lib.load()
    src = _need(src, "src")
    grad_out = _need(grad_out, "grad_out")
    theta = _need(theta, "theta")
    B, C, H, W = src.shape
    n_out, C2, OH, OW = grad_out.shape
    assert C2 == C
    E = theta.shape[0]
    gidx, p_gidx = _opt(gidx, "gidx", torch.int32)
    flags, p_flags = _opt(flags, "flags", torch.int32)
    chan_map, p_map = _opt(chan_map, "chan_map", torch.int32)
    G = chan_map.shape[1] if chan_map is not None else 1
    if want_src and pad > 0 and gidx is not None and n_out == B and chan_map is None and not lib.eqa_get_option(0):
        # edge-padded transform (canonicalize): deterministic, atomics-free input gradient in two steps -- the gather adjoint
        # on the padded FRAME as its source (dL/d frame), then the adjoint of the replicate padding (strips and corners folded
        # onto the image borders).  The transform gradient, if wanted, comes from the ordinary call below without grad_src.
        Hp, Wp = H + 2 * pad, W + 2 * pad
        g_frame = torch.empty((B, C, Hp, Wp), dtype=torch.float32, device=src.device)
        with torch.cuda.device(src.device):
            st = lib.eqa_group_action_bwd(g_frame.data_ptr(), grad_out.data_ptr(), p_gidx, theta.data_ptr(), p_flags, None,
                                          g_frame.data_ptr(), None, E, 1, n_out, B, C, Hp, Wp, 0, OH, OW, top_left[0], top_left[1],
                                          _stream())
            _lib.check(st, "eqa_group_action_bwd (frame gather)")
            g_src = torch.empty_like(src)
            ws = torch.empty((lib.eqa_fold_edge_pad_workspace_bytes(B * C, H, W, pad) // 4,), dtype=torch.float32, device=src.device)
            _lib.check(lib.eqa_fold_edge_pad(g_frame.data_ptr(), g_src.data_ptr(), ws.data_ptr(), B * C, H, W, pad, _stream()),
                       "eqa_fold_edge_pad")
        if not (want_angle or want_theta):
            return g_src, None
        _, g_t = group_action_bwd(src, grad_out, gidx, theta, flags, chan_map, pad, top_left, False, want_angle, want_theta)
        return g_src, g_t
    g_src = torch.zeros_like(src) if want_src else None
    tiles = lib.eqa_group_action_bwd_tiles(OH, OW)
    if want_theta:
        partial = torch.empty((n_out, tiles, 6), dtype=torch.float32, device=src.device)
        with torch.cuda.device(src.device):
            st = lib.eqa_group_action_bwd_theta(src.data_ptr(), grad_out.data_ptr(), p_gidx, theta.data_ptr(), p_flags, p_map,
                                                g_src.data_ptr() if want_src else None, partial.data_ptr(),
                                                E, G, n_out, B, C, H, W, pad, OH, OW, top_left[0], top_left[1], _stream())
        _lib.check(st, "eqa_group_action_bwd_theta")
        return g_src, partial.sum(dim=1)
    partial = torch.empty((n_out, tiles), dtype=torch.float32, device=src.device) if want_angle else None
    with torch.cuda.device(src.device):
        st = lib.eqa_group_action_bwd(src.data_ptr(), grad_out.data_ptr(), p_gidx, theta.data_ptr(), p_flags, p_map,
                                      g_src.data_ptr() if want_src else None, partial.data_ptr() if want_angle else None,
                                      E, G, n_out, B, C, H, W, pad, OH, OW, top_left[0], top_left[1], _stream())
    _lib.check(st, "eqa_group_action_bwd")
    g_angle = partial.sum(dim=1) * (3.141592653589793 / 180.0) if want_angle else None
    return g_src, g_angle


# Window-bound hints: device address of an element table -> the most source rows a 32 x 32 output tile can sample under ANY of its
# elements (images.utils.device_tables registers 35 for right-angle groups on square frames).  A registry keyed by the table's
# storage, not an attribute on the tensor: .to() / .clone() / tracing drop attributes silently, and a copy at another address
# simply has no hint.  The hint only sizes the LDS reservation (eqa_group_action_fwd_hint); a tile whose window exceeds it takes
# the direct gather path, so a stale or wrong hint costs time, never correctness.
#  keyed by (device, address, element count) and dropped when the registered tensor dies: the caching allocator hands a
# freed table's address to the next allocation, and another table at that address must not inherit the hint (it would push every
# oversized tile onto the slow path without anyone noticing).
_window_hints: dict = {}


def _hint_key(theta: torch.Tensor):
    return (theta.device.index, theta.data_ptr(), theta.numel())


def register_window_hint(theta: torch.Tensor, max_window_rows: int) -> None:
    import weakref

    key = _hint_key(theta)
    _window_hints[key] = int(max_window_rows)
    weakref.finalize(theta, _window_hints.pop, key, None)


def _window_hint(theta: torch.Tensor, explicit: Optional[int]) -> int:
    return int(explicit) if explicit is not None else _window_hints.get(_hint_key(theta), 0)


def canon_transform(x: torch.Tensor, gidx: torch.Tensor, theta: torch.Tensor, flags: Optional[torch.Tensor], pad: int,
                    max_window: Optional[int] = None) -> torch.Tensor:
    """I5: fused pad(edge) -> [hflip] -> rotate -> center-crop (eqa_canon_transform_fwd).  ``max_window``: bound on a tile's source
    window rows (0 = none; default: what was registered for this table)."""
    lib = _lib.load()
    x = _need(x, "x")
    gidx = _need(gidx, "gidx", torch.int32)
    theta = _need(theta, "theta")
    flags, p_flags = _opt(flags, "flags", torch.int32)
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    hint = _window_hint(theta, max_window)
    with torch.cuda.device(x.device), _timed("canon_transform"):
        if hint > 0 and B > 0:
            st = lib.eqa_group_action_fwd_hint(x.data_ptr(), y.data_ptr(), gidx.data_ptr(), theta.data_ptr(), p_flags, None,
                                               theta.shape[0], 1, B, B, C, H, W, pad, H, W, pad, pad, hint, _stream())
        else:
            st = lib.eqa_canon_transform_fwd(x.data_ptr(), y.data_ptr(), gidx.data_ptr(), theta.data_ptr(), p_flags,
                                             theta.shape[0], B, C, H, W, pad, _stream())
    _lib.check(st, "eqa_canon_transform_fwd")
    return y


def invert_action(f: torch.Tensor, gidx: torch.Tensor, theta: torch.Tensor, flags: Optional[torch.Tensor],
                  chan_map: Optional[torch.Tensor], max_window: Optional[int] = None) -> torch.Tensor:
    """I7: rotate(+theta) zero-corner -> flip -> regular-representation roll (eqa_invert_action_fwd)."""
    lib = _lib.load()
    f = _need(f, "feature_map")
    gidx = _need(gidx, "gidx", torch.int32)
    theta = _need(theta, "theta")
    flags, p_flags = _opt(flags, "flags", torch.int32)
    chan_map, p_map = _opt(chan_map, "chan_map", torch.int32)
    G = chan_map.shape[1] if chan_map is not None else 1
    B, C, H, W = f.shape
    out = torch.empty_like(f)
    hint = _window_hint(theta, max_window)
    with torch.cuda.device(f.device), _timed("invert_action"):
        if hint > 0 and B > 0:
            st = lib.eqa_group_action_fwd_hint(f.data_ptr(), out.data_ptr(), gidx.data_ptr(), theta.data_ptr(), p_flags, p_map,
                                               theta.shape[0], G, B, B, C, H, W, 0, H, W, 0, 0, hint, _stream())
        else:
            st = lib.eqa_invert_action_fwd(f.data_ptr(), out.data_ptr(), gidx.data_ptr(), theta.data_ptr(), p_flags, p_map,
                                           theta.shape[0], G, B, C, H, W, _stream())
    _lib.check(st, "eqa_invert_action_fwd")
    return out


def group_action_pair(x: torch.Tensor, f: torch.Tensor, gidx: torch.Tensor, theta_canon: torch.Tensor,
                      flags_canon: Optional[torch.Tensor], pad: int, theta_inv: torch.Tensor, flags_inv: Optional[torch.Tensor],
                      chan_map: Optional[torch.Tensor]):
    """I5 + I7 in one launch (eqa_group_action_pair): (canon_transform(x, ...), invert_action(f, ...)) for the same group
    index, bit-identical to the two separate calls.  x:(B,C,H,W), f:(B,Cf,H,W)."""
    lib = _lib.load()
    x, f = _need(x, "x"), _need(f, "feature_map")
    gidx = _need(gidx, "gidx", torch.int32)
    theta_canon, theta_inv = _need(theta_canon, "theta_canon"), _need(theta_inv, "theta_inv")
    flags_canon, p_fc = _opt(flags_canon, "flags_canon", torch.int32)
    flags_inv, p_fi = _opt(flags_inv, "flags_inv", torch.int32)
    chan_map, p_map = _opt(chan_map, "chan_map", torch.int32)
    G = chan_map.shape[1] if chan_map is not None else 1
    B, C, H, W = x.shape
    if f.shape[0] != B or tuple(f.shape[2:]) != (H, W) or theta_canon.shape[0] != theta_inv.shape[0]:
        raise ValueError(f"group_action_pair: x {tuple(x.shape)} and f {tuple(f.shape)} must share batch and spatial size, and the tables their element count")
    y, out = torch.empty_like(x), torch.empty_like(f)
    with torch.cuda.device(x.device), _timed("group_action_pair"):
        st = lib.eqa_group_action_pair(x.data_ptr(), y.data_ptr(), theta_canon.data_ptr(), p_fc, pad, C, f.data_ptr(), out.data_ptr(),
                                       theta_inv.data_ptr(), p_fi, p_map, G, f.shape[1], gidx.data_ptr(), theta_canon.shape[0], B, H, W,
                                       _stream())
    _lib.check(st, "eqa_group_action_pair")
    return y, out


def orbit_expand(x: torch.Tensor, theta: torch.Tensor, flags: Optional[torch.Tensor], pad: int) -> torch.Tensor:
    """I8: all E group views of every image, element-major (eqa_orbit_expand_fwd)."""
    lib = _lib.load()
    x = _need(x, "x")
    theta = _need(theta, "theta")
    flags, p_flags = _opt(flags, "flags", torch.int32)
    B, C, S, S2 = x.shape
    if S != S2:
        raise ValueError("orbit_expand expects square images (the reference crops to a square resize_shape)")
    E = theta.shape[0]
    y = torch.empty((E * B, C, S, S), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.eqa_orbit_expand_fwd(x.data_ptr(), y.data_ptr(), theta.data_ptr(), p_flags, E, B, C, S, pad, _stream())
    _lib.check(st, "eqa_orbit_expand_fwd")
    return y


def group_pool_argmax(feature_map: torch.Tensor, want_index: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """I3+I4: (B, Cf, G, H', W') -> activations (B, G) [mean over Cf, H', W'] and argmax index (B,) int32."""
    lib = _lib.load()
    feature_map = _need(feature_map, "feature_map")
    B, Cf, G, Hf, Wf = feature_map.shape
    HW = Hf * Wf
    act = torch.empty((B, G), dtype=torch.float32, device=feature_map.device)
    gidx = torch.empty((B,), dtype=torch.int32, device=feature_map.device) if want_index else None
    nbytes = lib.eqa_group_pool_workspace_bytes(B, Cf, G, HW)
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=feature_map.device)
    with torch.cuda.device(feature_map.device), _timed("group_pool"):
        st = lib.eqa_group_pool_argmax(feature_map.data_ptr(), act.data_ptr(), gidx.data_ptr() if want_index else None,
                                       ws.data_ptr(), B, Cf, G, HW, _stream())
    _lib.check(st, "eqa_group_pool_argmax")
    return act, gidx


def window_sums(x: torch.Tensor, k: int, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                relu: bool = False) -> torch.Tensor:
    """(B,C,H,W) fp32 -> (B,C,k,k) fp64 sums of act(x) over the k*k shifted (H-k+1)x(W-k+1) windows
    (eqa_window_sums); act(t) = [relu](scale[c]*t + shift[c])."""
    lib = _lib.load()
    B, C, H, W = x.shape
    scale, p_scale = _opt(scale, "scale", torch.float32)
    shift, p_shift = _opt(shift, "shift", torch.float32)
    out = torch.empty((B, C, k, k), dtype=torch.float64, device=x.device)
    if (x.is_cuda and x.dtype == torch.float32 and C % 4 == 0 and not x.is_contiguous()
            and x.is_contiguous(memory_format=torch.channels_last) and H > 2 * (k - 1) and W > 2 * (k - 1)):
        # (B,H,W,C) in memory: the channels-last kernels read it as it is
        ws = torch.empty((max(lib.eqa_window_sums_nhwc_workspace_bytes(B, C, H, k), 4) // 4,), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device), _timed("window_sums"):
            st = lib.eqa_window_sums_nhwc(x.data_ptr(), p_scale, p_shift, int(relu), out.data_ptr(), ws.data_ptr(), B, C, H, W, k, _stream())
        _lib.check(st, "eqa_window_sums_nhwc")
        return out
    x = _need(x, "x")
    with torch.cuda.device(x.device), _timed("window_sums"):
        st = lib.eqa_window_sums(x.data_ptr(), p_scale, p_shift, int(relu), out.data_ptr(), B, C, H, W, k, _stream())
    _lib.check(st, "eqa_window_sums")
    return out


def group_argmax(act: torch.Tensor) -> torch.Tensor:
    """I4: first-maximum argmax over the group axis, (B, G) -> (B,) int32."""
    lib = _lib.load()
    act = _need(act.detach(), "group_activations")
    B, G = act.shape
    gidx = torch.empty((B,), dtype=torch.int32, device=act.device)
    with torch.cuda.device(act.device):
        st = lib.eqa_group_argmax(act.data_ptr(), gidx.data_ptr(), B, G, _stream())
    _lib.check(st, "eqa_group_argmax")
    return gidx


def so3_rotate(x: torch.Tensor, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """P4: y[b] = R[b] @ x[b] (or R[b]^T @ x[b]);  x:(B,3,N), R:(B,3,3)."""
    lib = _lib.load()
    x = _need(x, "x")
    R = _need(R, "R")
    B, three, N = x.shape
    if three != 3 or tuple(R.shape) != (B, 3, 3):
        raise ValueError("so3_rotate expects x:(B,3,N) and R:(B,3,3)")
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = lib.eqa_so3_rotate(x.data_ptr(), R.data_ptr(), y.data_ptr(), B, N, int(transpose), _stream())
    _lib.check(st, "eqa_so3_rotate")
    return y


def gram_schmidt(v: torch.Tensor) -> torch.Tensor:
    """P3: batched classical Gram-Schmidt on the rows of (B,3,3)."""
    lib = _lib.load()
    v = _need(v, "vectors")
    if v.dim() != 3 or v.shape[1:] != (3, 3):
        raise ValueError("gram_schmidt expects (B,3,3)")
    out = torch.empty_like(v)
    with torch.cuda.device(v.device):
        st = lib.eqa_gram_schmidt(v.data_ptr(), out.data_ptr(), v.shape[0], _stream())
    _lib.check(st, "eqa_gram_schmidt")
    return out


def _vnsmall_args(what: str, x: torch.Tensor, params: torch.Tensor, pooling: str):
    """The argument check of the two fused VNSmall ops -> (x, params, B, N)."""
    x = _need(x, "point_cloud")
    params = _need(params, "params")
    B, three, N = x.shape
    if pooling not in ("mean", "max"):
        raise ValueError(f"Pooling type {pooling} not supported")
    if three != 3 or params.numel() != (VNSMALL_PARAMS if pooling == "mean" else VNSMALL_PARAMS_MAX):
        raise ValueError(f"{what} expects x:(B,3,N) and {VNSMALL_PARAMS} (mean) / {VNSMALL_PARAMS_MAX} (max) packed parameters")
    return x, params, B, N


def vnsmall_forward(x: torch.Tensor, params: torch.Tensor, k: int = 20, pooling: str = "mean") -> torch.Tensor:
    """P1+P2 fused: (B,3,N) point clouds + packed VNSmall parameters -> (B,3,3) equivariant vectors (eqa_vnsmall_fwd).
    ``pooling`` "mean" (1310 packed floats) or "max" (1751: + the pooling layer's 21 x 21 direction map)."""
    lib = _lib.load()
    x, params, B, N = _vnsmall_args("vnsmall_forward", x, params, pooling)
    out = torch.empty((B, 3, 3), dtype=torch.float32, device=x.device)
    ws = torch.empty((max(lib.eqa_vnsmall_workspace_bytes(B, N), 4) // 4,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("vnsmall_fwd"):
        st = lib.eqa_vnsmall_fwd(x.data_ptr(), params.data_ptr(), out.data_ptr(), ws.data_ptr(), B, N, k, int(pooling == "max"), _stream())
    _lib.check(st, "eqa_vnsmall_fwd")
    return out


def vnsmall_canonicalize(x: torch.Tensor, params: torch.Tensor, k: int = 20, pooling: str = "mean"):
    """P1-P4 in two launches (eqa_vnsmall_canonicalize): (B,3,N) clouds -> (network output vectors (B,3,3), their Gram-Schmidt
    frame R (B,3,3), canonical clouds R x (B,3,N))."""
    lib = _lib.load()
    x, params, B, N = _vnsmall_args("vnsmall_canonicalize", x, params, pooling)
    vec = torch.empty((B, 3, 3), dtype=torch.float32, device=x.device)
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    ws = torch.empty((max(lib.eqa_vnsmall_workspace_bytes(B, N), 4) // 4,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("vnsmall_fwd"):
        st = lib.eqa_vnsmall_canonicalize(x.data_ptr(), params.data_ptr(), vec.data_ptr(), R.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                          B, N, k, int(pooling == "max"), _stream())
    _lib.check(st, "eqa_vnsmall_canonicalize")
    return vec, R, y


def crop_resize_aa(x: torch.Tensor, tables, out_hw: Tuple[int, int], pixels: bool = True) -> torch.Tensor:
    """I1: centre crop + antialiased bilinear resize in one kernel (eqa_crop_resize_aa).  ``tables`` from
    ``geometry.aa_resize_tables`` already moved to x.device.  ``pixels``: the consumer reads channels-last (the canonicalization
    networks' lifting kernels): where eqa_crop_resize_aa_nhwc takes the shape the result is channels-last, same values."""
    lib = _lib.load()
    x = _need(x, "x")
    wx, x0, wy, y0, K, max_rows, x_begin, x_span = tables
    B, C, H, W = x.shape
    OH, OW = out_hw
    if pixels and os.environ.get("EQA_HEAD_FUSED", "1") != "0" and B > 0 and C in (1, 3) and x.data_ptr() % 16 == 0:
        # channels-last, with the bound the fused lifting kernel scales its pixels by (eqa_crop_resize_aa_nhwc): the network's
        # .contiguous(channels_last) returns this very tensor, and `crop_absmax_slots` hands the bound over while it is unchanged
        nslots = lib.eqa_crop_resize_aa_nhwc_slots(B, C, H, W, OH, OW, K, max_rows, x_begin, x_span)
        if nslots > 0:
            y = torch.empty((B, OH, OW, C), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
            slots = torch.empty((nslots,), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device), _timed("crop_resize_aa_nhwc"):
                st = lib.eqa_crop_resize_aa_nhwc(x.data_ptr(), y.data_ptr(), wx.data_ptr(), x0.data_ptr(), wy.data_ptr(), y0.data_ptr(),
                                                 B, C, H, W, OH, OW, K, max_rows, x_begin, x_span, slots.data_ptr(), _stream())
            _lib.check(st, "eqa_crop_resize_aa_nhwc")
            y._eqa_absmax = (slots, _stamp((y,)))
            return y
    y = torch.empty((B, C, out_hw[0], out_hw[1]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("crop_resize_aa"):
        st = lib.eqa_crop_resize_aa(x.data_ptr(), y.data_ptr(), wx.data_ptr(), x0.data_ptr(), wy.data_ptr(), y0.data_ptr(),
                                    B * C, H, W, out_hw[0], out_hw[1], K, max_rows, x_begin, x_span, _stream())
    _lib.check(st, "eqa_crop_resize_aa")
    return y


def crop_absmax_slots(y: torch.Tensor) -> Optional[torch.Tensor]:
    """The floats whose maximum is max |y|, if `y` is a channels-last result of `crop_resize_aa` that nothing has written to since
    (the rule of common/derived.py: the same object, at the same ``_version``, over the same ``data_ptr()``); else None."""
    kept = getattr(y, "_eqa_absmax", None)
    if kept is None or kept[1] != _stamp((y,)):
        return None
    return kept[0]


def mask_action_nearest(masks: torch.Tensor, eidx: torch.Tensor, rtheta: torch.Tensor, flags: Optional[torch.Tensor]) -> torch.Tensor:
    """I6: nearest-neighbour rotation (+ optional pre-flip) of (n,H,W) uint8 masks, element index per mask."""
    lib = _lib.load()
    masks = _need(masks, "masks", torch.uint8)
    eidx = _need(eidx, "eidx", torch.int32)
    rtheta = _need(rtheta, "rtheta")
    flags, p_flags = _opt(flags, "flags", torch.int32)
    n, H, W = masks.shape
    out = torch.empty_like(masks)
    with torch.cuda.device(masks.device), _timed("mask_action"):
        st = lib.eqa_mask_action_nearest(masks.data_ptr(), out.data_ptr(), eidx.data_ptr(), rtheta.data_ptr(), p_flags,
                                         rtheta.shape[0], n, H, W, _stream())
    _lib.check(st, "eqa_mask_action_nearest")
    return out


_plane_tables: dict = {}


def mask_action_nearest_planes(mask_list, eidx: torch.Tensor, rtheta: torch.Tensor, flags: Optional[torch.Tensor]) -> torch.Tensor:
    """I6 for a LIST of per-sample (n_t, H, W) uint8 mask tensors: one launch over all planes, read through a table of plane
    pointers (eqa_mask_action_nearest_planes) instead of a concatenated copy.  Returns one (sum n_t, H, W) tensor."""
    lib = _lib.load()
    eidx = _need(eidx, "eidx", torch.int32)
    rtheta = _need(rtheta, "rtheta")
    flags, p_flags = _opt(flags, "flags", torch.int32)
    masks = [_need(m, "masks", torch.uint8) for m in mask_list]
    H, W = masks[0].shape[-2:]
    ptrs = tuple(m.data_ptr() + k * H * W for m in masks for k in range(m.shape[0]))
    n = len(ptrs)
    dev = masks[0].device
    # the pointer table is uploaded once per set of mask tensors: a loop that re-uses its target buffers (and a captured
    # hipGraph, which must not contain a pageable host-to-device copy) finds it on the device
    key = (ptrs, str(dev))
    table = _plane_tables.get(key)
    if table is None:
        if len(_plane_tables) >= 64:
            _plane_tables.clear()
        table = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        _plane_tables[key] = table
    out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("mask_action"):
        st = lib.eqa_mask_action_nearest_planes(table.data_ptr(), out.data_ptr(), eidx.data_ptr(), rtheta.data_ptr(), p_flags,
                                                rtheta.shape[0], n, H, W, _stream())
    _lib.check(st, "eqa_mask_action_nearest_planes")
    return out


def boxes_action(boxes: torch.Tensor, img_of_box: torch.Tensor, rotation_deg: torch.Tensor, width: float,
                 flip_all: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """I6: every (n,4) xyxy box flipped (if ``flip_all``) and rotated by its image's angle about (width/2, width/2), one
    launch (eqa_boxes_action).  Returns (new boxes, boxes after the flip or None)."""
    lib = _lib.load()
    boxes = _need(boxes, "boxes")
    img_of_box = _need(img_of_box, "img_of_box", torch.int32)
    rotation_deg = _need(rotation_deg, "rotation_deg")
    out = torch.empty_like(boxes)
    flipped = torch.empty_like(boxes) if flip_all else None
    with torch.cuda.device(boxes.device):
        st = lib.eqa_boxes_action(boxes.data_ptr(), img_of_box.data_ptr(), rotation_deg.data_ptr(),
                                  flipped.data_ptr() if flip_all else None, out.data_ptr(), boxes.shape[0], float(width),
                                  int(flip_all), _stream())
    _lib.check(st, "eqa_boxes_action")
    return out, flipped


def conv_s2_supported(cin: int, cout: int, k: int, pad: int, planar: bool) -> bool:
    return bool(_lib.load().eqa_conv_s2_supported(cin, cout, k, pad, int(planar)))


def pack_conv_s2_weights(w: torch.Tensor, planar: bool) -> torch.Tensor:
    """(Cout, Cin, K, K) filters -> the operand order of eqa_conv_s2 (layouts: include/eqa_hip.h)."""
    Cout, Cin, K, _ = w.shape
    if planar:
        wp = torch.zeros(Cout, 4, K, K, dtype=w.dtype, device=w.device)
        wp[:, :Cin] = w
        return wp.permute(2, 3, 1, 0).reshape(K * K, 4, Cout // 16, 16).permute(0, 2, 1, 3).contiguous()
    t = w.permute(2, 3, 1, 0).reshape(K * K, Cin // 16, 4, 4, Cout // 16, 16)      # tap, chunk, kq, s, n, j
    return t.permute(0, 1, 4, 2, 5, 3).contiguous()                                  # tap, chunk, n, kq, j, s


def conv_s2(x: torch.Tensor, wp: torch.Tensor, bias: Optional[torch.Tensor], gelu: bool, cout: int, k: int, pad: int,
            planar: bool) -> torch.Tensor:
    """Stride-2 k x k convolution (+ bias, + exact GELU) on the fp32 MFMA (eqa_conv_s2).  planar: x (B,Cin<=4,H,W) contiguous;
    else x is a (B,H,W,Cin) contiguous tensor.  Returns (B,OH,OW,Cout) contiguous (channels-last data)."""
    lib = _lib.load()
    x, wp = _need(x, "x"), _need(wp, "wp")
    bias, p_bias = _opt(bias, "bias", torch.float32)
    if planar:
        B, cin, H, W = x.shape
    else:
        B, H, W, cin = x.shape
    OH, OW = (H + 2 * pad - k) // 2 + 1, (W + 2 * pad - k) // 2 + 1
    y = torch.empty((B, OH, OW, cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("conv_s2"):
        st = lib.eqa_conv_s2(x.data_ptr(), wp.data_ptr(), p_bias, int(gelu), y.data_ptr(), B, cin, H, W, cout, k, pad, int(planar), _stream())
    _lib.check(st, "eqa_conv_s2")
    return y


def pack_conv_s2_dgrad_weights(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, K, K) filters -> the operand order of eqa_conv_s2_dgrad: (K*K, Cout/16, Cin/16, 4 [kq], 16 [j], 4 [s]) holding
    w[16 cc + 4 kq + s][16 n + j][u][v]."""
    Cout, Cin, K, _ = w.shape
    t = w.permute(2, 3, 0, 1).reshape(K * K, Cout // 16, 4, 4, Cin // 16, 16)      # tap, cc, kq, s, n, j
    return t.permute(0, 1, 4, 2, 5, 3).contiguous()                                  # tap, cc, n, kq, j, s


def conv_s2_train_supported(cin: int, cout: int, k: int, pad: int, planar: bool) -> bool:
    lib = _lib.load()
    return bool(lib.eqa_conv_s2_wgrad_supported(cin, cout, k, pad, int(planar))) and (planar or bool(lib.eqa_conv_s2_dgrad_supported(cin, cout, k, pad)))


def conv_s2_wgrad(x: torch.Tensor, dz: torch.Tensor, k: int, pad: int, planar: bool) -> torch.Tensor:
    """Filter gradient of eqa_conv_s2 (eqa_conv_s2_wgrad): x the layer's input (planar: (B,Cin,H,W); else (B,H,W,Cin)),
    dz (B,OH,OW,Cout) -> (Cout,Cin,K,K)."""
    lib = _lib.load()
    x, dz = _need(x, "x"), _need(dz, "dz")
    if planar:
        B, cin, H, W = x.shape
    else:
        B, H, W, cin = x.shape
    cout = dz.shape[-1]
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
    ws = torch.empty((max(lib.eqa_conv_s2_wgrad_workspace_bytes(B, cin, H, W, cout, k, pad, int(planar)), 16) // 4,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("conv_s2_wgrad"):
        st = lib.eqa_conv_s2_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), B, cin, H, W, cout, k, pad, int(planar), _stream())
    _lib.check(st, "eqa_conv_s2_wgrad")
    return dw


def conv_s2_dgrad(dz: torch.Tensor, wd: torch.Tensor, in_hw: Tuple[int, int], cin: int, k: int, pad: int) -> torch.Tensor:
    """Data gradient of eqa_conv_s2 for a channels-last layer (eqa_conv_s2_dgrad): dz (B,OH,OW,Cout), wd from
    ``pack_conv_s2_dgrad_weights`` -> (B,H,W,Cin)."""
    lib = _lib.load()
    dz, wd = _need(dz, "dz"), _need(wd, "wd")
    B, cout = dz.shape[0], dz.shape[-1]
    dx = torch.empty((B, in_hw[0], in_hw[1], cin), dtype=torch.float32, device=dz.device)
    with torch.cuda.device(dz.device), _timed("conv_s2_dgrad"):
        st = lib.eqa_conv_s2_dgrad(dz.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, cin, in_hw[0], in_hw[1], cout, k, pad, _stream())
    _lib.check(st, "eqa_conv_s2_dgrad")
    return dx


def _bn_act_partials(z: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    npix, C = z.shape
    part = torch.empty((max(lib.eqa_bn_act_partial_blocks(npix), 1), C, 2), dtype=torch.float64, device=z.device)
    with torch.cuda.device(z.device), _timed("bn_act_stats"):
        st = lib.eqa_bn_act_stats(z.data_ptr(), part.data_ptr(), npix, C, _stream())
    _lib.check(st, "eqa_bn_act_stats")
    return part


def bn_batch_stats(z: torch.Tensor):
    """Per-channel batch mean and BIASED variance (fp64) of a channels-last (npix, C) view (eqa_bn_act_stats: fp32 sums inside
    blocks of up to 1024 pixels -- shifted by the block's first pixel, so that a large mean does not cancel the variance --, fp64 across them)."""
    z = _need(z, "z")
    sums = _bn_act_partials(z).sum(0)
    mean = sums[:, 0] / z.shape[0]
    var = (sums[:, 1] / z.shape[0] - mean * mean).clamp_min(0.0)
    return mean, var


def bn_fold_batch_stats(z: torch.Tensor, bn: torch.nn.modules.batchnorm._BatchNorm):
    """Batch statistics of a channels-last (npix, C) view folded with the module's affine parameters, the module's running
    statistics updated as a training-mode forward of nn.BatchNorm*d does -- eqa_bn_act_stats + ONE eqa_bn_act_finalize launch
    (the same through torch: ~25 element-wise launches on C-sized tensors) -> (scale, shift, mean, rstd) fp32."""
    from equiadapt_amd.common.utils import mark_written

    lib = _lib.load()
    z = _need(z, "z")
    npix, C = z.shape
    part = _bn_act_partials(z)
    out = torch.empty((4, C), dtype=torch.float32, device=z.device)
    track = bn.track_running_stats and bn.running_mean is not None
    momentum = 0.0
    if track:
        with torch.no_grad():
            bn.num_batches_tracked += 1
        momentum = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
    with torch.cuda.device(z.device):
        st = lib.eqa_bn_act_finalize(part.data_ptr(), npix, C, bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), float(momentum),
                                     bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _stream())
    _lib.check(st, "eqa_bn_act_finalize")
    if track:
        mark_written(bn.running_mean, bn.running_var)
    return out[0], out[1], out[2], out[3]


def bn_act_fwd(z: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, rowscale: Optional[torch.Tensor], act: int) -> torch.Tensor:
    """y = rowscale[p] * act(scale[c] z + shift[c]) on a channels-last (npix, C) view (eqa_bn_act_fwd); act 0 = GELU (erf), 1 = ReLU."""
    lib = _lib.load()
    z, scale, shift = _need(z, "z"), _need(scale, "scale"), _need(shift, "shift")
    rowscale, p_rs = _opt(rowscale, "rowscale", torch.float32)
    npix, C = z.shape
    y = torch.empty_like(z)
    with torch.cuda.device(z.device), _timed("bn_act_fwd"):
        st = lib.eqa_bn_act_fwd(z.data_ptr(), scale.data_ptr(), shift.data_ptr(), p_rs, y.data_ptr(), npix, C, act, _stream())
    _lib.check(st, "eqa_bn_act_fwd")
    return y


def bn_act_bwd(gy: torch.Tensor, z: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
               gamma: torch.Tensor, rowscale: Optional[torch.Tensor], act: int):
    """Backward of batch-norm (batch statistics) + activation on (npix, C): -> (dz, dgamma, dbeta) (eqa_bn_act_bwd_reduce / _apply)."""
    lib = _lib.load()
    gy, z = _need(gy, "gy"), _need(z, "z")
    rowscale, p_rs = _opt(rowscale, "rowscale", torch.float32)
    npix, C = z.shape
    part = torch.empty((max(lib.eqa_bn_act_partial_blocks(npix), 1), C, 2), dtype=torch.float64, device=z.device)
    with torch.cuda.device(z.device), _timed("bn_act_bwd_reduce"):
        st = lib.eqa_bn_act_bwd_reduce(gy.data_ptr(), z.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p_rs,
                                       part.data_ptr(), npix, C, act, _stream())
    _lib.check(st, "eqa_bn_act_bwd_reduce")
    coef = torch.empty((5, C), dtype=torch.float32, device=z.device)          # dgamma, dbeta, gscale, m1, m2
    with torch.cuda.device(z.device):
        st = lib.eqa_bn_act_bwd_finalize(part.data_ptr(), npix, C, gamma.data_ptr(), rstd.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(),
                                         coef[2].data_ptr(), coef[3].data_ptr(), coef[4].data_ptr(), _stream())
    _lib.check(st, "eqa_bn_act_bwd_finalize")
    dgamma, dbeta, gscale, m1, m2 = coef[0], coef[1], coef[2], coef[3], coef[4]
    dz = torch.empty_like(z)
    with torch.cuda.device(z.device), _timed("bn_act_bwd_apply"):
        st = lib.eqa_bn_act_bwd_apply(gy.data_ptr(), z.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p_rs,
                                      gscale.data_ptr(), m1.data_ptr(), m2.data_ptr(), dz.data_ptr(), npix, C, act, _stream())
    _lib.check(st, "eqa_bn_act_bwd_apply")
    return dz, dgamma, dbeta


def _need_nhwc(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError(f"{name} must be a channels-last (B,C,H,W) fp32 tensor on the device")
    return t


def inner_bn_stats(h: torch.Tensor) -> torch.Tensor:
    """Channels-last (B,C,H,W) -> (eqa_bn_partial_blocks, C, 2) fp64 partial sums of the per-channel sum / sum of squares (eqa_bn_stats_nhwc)."""
    lib = _lib.load()
    h = _need_nhwc(h, "h")
    B, C, H, W = h.shape
    npix = B * H * W
    part = torch.empty((lib.eqa_bn_partial_blocks(npix), C, 2), dtype=torch.float64, device=h.device)
    with torch.cuda.device(h.device):
        st = lib.eqa_bn_stats_nhwc(h.data_ptr(), part.data_ptr(), npix, C, _stream())
    _lib.check(st, "eqa_bn_stats_nhwc")
    return part


def inner_bn_relu_dropout(h: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """y = dropout(relu(scale[c] h + shift[c]), p), channels-last (B,C,H,W); mask: a hash of (seed, element index) (eqa_bn_relu_dropout_nhwc)."""
    lib = _lib.load()
    h, scale, shift = _need_nhwc(h, "h"), _need(scale, "scale"), _need(shift, "shift")
    B, C, H, W = h.shape
    y = torch.empty_like(h)
    with torch.cuda.device(h.device):
        st = lib.eqa_bn_relu_dropout_nhwc(h.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), B * H * W, C, float(p), seed, _stream())
    _lib.check(st, "eqa_bn_relu_dropout_nhwc")
    return y


def _inner_bn_bwd(stage: str, g, h, mean_c, rstd_c, abd, out, scale, shift, p: float, seed: int, k: int) -> torch.Tensor:
    """One backward pass (stage: "reduce" | "apply") of dropout(relu(InnerBatchNorm(h))) into out.  k == 0: g is the channels-last
    (B,C,H,W) upstream gradient (eqa_bn_bwd_*_nhwc; the block's output they also take is NULL: "kept and positive" is recomputed);
    k > 0: g is the window sums' (B, 2k-1, 2k-1, C) class table (eqa_bn_bwd_*_nhwc_wsgrad)."""
    B, C, H, W = _need_nhwc(h, "h").shape
    if k > 0:
        if _need(g, "table").shape != (B, 2 * k - 1, 2 * k - 1, C) or not g.is_contiguous():
            raise ValueError(f"the class table of k = {k} on {tuple(h.shape)} is a contiguous (B, 2k-1, 2k-1, C) tensor, got {tuple(g.shape)}")
        name, head, dims = f"eqa_bn_bwd_{stage}_nhwc_wsgrad", (g.data_ptr(),), (B, H, W, C, k)
    else:
        if _need_nhwc(g, "g").shape != h.shape:
            raise ValueError(f"g {tuple(g.shape)} does not match h {tuple(h.shape)}")
        name, head, dims = f"eqa_bn_bwd_{stage}_nhwc", (g.data_ptr(), None), (B * H * W, C)
    vecs = [_need(v, "per-channel vector") for v in (mean_c, rstd_c, *abd, scale, shift)]
    ptr = [v.data_ptr() for v in vecs]
    with torch.cuda.device(h.device):
        st = getattr(_lib.load(), name)(*head, h.data_ptr(), *ptr[:-2], float(p), out.data_ptr(), *dims, *ptr[-2:], seed, _stream())
    _lib.check(st, name)
    return out


def inner_bn_bwd_reduce(g, h, mean_c, rstd_c, scale, shift, p: float, seed: int, k: int = 0) -> torch.Tensor:
    """First backward pass of the hidden block: (eqa_bn_partial_blocks, C, 2) fp64 partial sums of the per-channel sum of the gradient
    behind mask and ReLU and of its product with x-hat (g, k: `_inner_bn_bwd`)."""
    B, C, H, W = h.shape
    part = torch.empty((_lib.load().eqa_bn_partial_blocks(B * H * W), C, 2), dtype=torch.float64, device=h.device)
    return _inner_bn_bwd("reduce", g, h, mean_c, rstd_c, (), part, scale, shift, p, seed, k)


def inner_bn_bwd_apply(g, h, mean_c, rstd_c, a, b, d, scale, shift, p: float, seed: int, k: int = 0) -> torch.Tensor:
    """Second backward pass: dh = a[c] (g' - b[c] - d[c] x-hat), g' the gradient behind mask and ReLU (g, k: `_inner_bn_bwd`)."""
    return _inner_bn_bwd("apply", g, h, mean_c, rstd_c, (a, b, d), torch.empty_like(h), scale, shift, p, seed, k)


def window_sums_nhwc_act(h: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, p: float, seed: int, k: int) -> torch.Tensor:
    """(B,C,k,k) fp64 window sums (`window_sums`) of `inner_bn_relu_dropout`'s output without that map being written: affine map,
    ReLU and the same dropout mask applied while the channels-last h is loaded (eqa_window_sums_nhwc_act)."""
    lib = _lib.load()
    h, scale, shift = _need_nhwc(h, "h"), _need(scale, "scale"), _need(shift, "shift")
    B, C, H, W = h.shape
    S = torch.empty((B, C, k, k), dtype=torch.float64, device=h.device)
    ws = torch.empty((max(lib.eqa_window_sums_nhwc_workspace_bytes(B, C, H, k), 4) // 4,), dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        st = lib.eqa_window_sums_nhwc_act(h.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, float(p), seed, S.data_ptr(), ws.data_ptr(),
                                          B, C, H, W, k, _stream())
    _lib.check(st, "eqa_window_sums_nhwc_act")
    return S


def affine_relu_rows(h: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """relu(h * scale[d] + shift[d]) on (rows, D) (eqa_affine_relu_rows): eval-mode BatchNorm1d + ReLU in one pass."""
    lib = _lib.load()
    h, scale, shift = _need(h, "h"), _need(scale, "scale"), _need(shift, "shift")
    rows, D = h.shape
    z = torch.empty_like(h)
    with torch.cuda.device(h.device):
        st = lib.eqa_affine_relu_rows(h.data_ptr(), scale.data_ptr(), shift.data_ptr(), z.data_ptr(), rows, D, _stream())
    _lib.check(st, "eqa_affine_relu_rows")
    return z


def cosine_group_activations(v: torch.Tensor, ref: torch.Tensor, num_group: int, eps: float = 1e-8) -> torch.Tensor:
    """(G*B, V) element-major embeddings, (V) reference -> (B, G) cosine similarities (eqa_cosine_group_activations)."""
    lib = _lib.load()
    v, ref = _need(v, "vector_out"), _need(ref.reshape(-1), "reference_vector")
    R, V = v.shape
    if R % num_group or ref.numel() != V:
        raise ValueError("cosine_group_activations expects (G*B, V) embeddings and a (V) reference vector")
    B = R // num_group
    act = torch.empty((B, num_group), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        st = lib.eqa_cosine_group_activations(v.data_ptr(), ref.data_ptr(), act.data_ptr(), B, num_group, V, float(eps), _stream())
    _lib.check(st, "eqa_cosine_group_activations")
    return act


def bias_relu_nhwc_(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """In place x = relu(x + bias[c]) on a channels-last (B,C,H,W) tensor (eqa_bias_relu_nhwc)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("bias_relu_nhwc_ expects a channels-last fp32 tensor on the device")
    bias = _need(bias, "bias")
    B, C, H, W = x.shape
    with torch.cuda.device(x.device), _timed("bias_relu"):
        st = lib.eqa_bias_relu_nhwc(x.data_ptr(), bias.data_ptr(), B * H * W, C, _stream())
    _lib.check(st, "eqa_bias_relu_nhwc")
    return x


def window_sums_gemv(S: torch.Tensor, weff: torch.Tensor, scale: float, shift) -> torch.Tensor:
    """(B, K) fp64 window sums x (E, K) fp64 mean-response weights -> (B, E) fp32 = scale * S @ weff^T + shift
    (eqa_window_sums_gemv).  `shift` may be a 0-dim device tensor (the bias mean): it is read without a host sync only
    if it already is a Python float."""
    lib = _lib.load()
    S = _need(S, "S", torch.float64)
    weff = _need(weff, "weff", torch.float64)
    B, K = S.shape
    E = weff.shape[0]
    act = torch.empty((B, E), dtype=torch.float32, device=S.device)
    sh = shift if isinstance(shift, float) else 0.0
    with torch.cuda.device(S.device), _timed("sums_gemv"):
        st = lib.eqa_window_sums_gemv(S.data_ptr(), weff.data_ptr(), act.data_ptr(), B, K, E, float(scale), sh, _stream())
    _lib.check(st, "eqa_window_sums_gemv")
    if not isinstance(shift, float):
        act += shift.to(torch.float32)
    return act


def window_sums_tail_supported(C: int, k: int, E: int) -> bool:
    """Does `window_sums_tail` take a C-channel map in front of a k x k tail with E group elements?  (eqa_window_sums_tail keeps an
    image's window sums, totals and border rows in one block's LDS: 560 bytes per channel at k = 5.)"""
    return k in (3, 5) and 1 <= E <= 16 and C * (8 * k * k + 8 * (2 * k - 1) + 8 * (k - 1) * (2 * k - 1)) <= 152 * 1024


def window_sums_tail(part: torch.Tensor, nimg: int, C: int, k: int, nseg: int, sub: int, weff: torch.Tensor, scale: float, shift: float,
                     rot_table: torch.Tensor, ref_table: Optional[torch.Tensor]):
    """Window-sum partials (nimg, nseg, C, 2k - 1) fp32, every segment in `sub` pieces -> (activations (nimg, E) fp32, first-maximum
    index (nimg,) int32, rotation (nimg,), reflection (nimg,) or None) in one launch (eqa_window_sums_tail): bit for bit what the
    finalize kernel, `window_sums_gemv`, `group_argmax` and ``torch.index_select`` on the tables give one after the other."""
    lib = _lib.load()
    weff = _need(weff, "weff", torch.float64)
    E, dev = weff.shape[0], part.device
    act = torch.empty((nimg, E), dtype=torch.float32, device=dev)
    gidx = torch.empty((nimg,), dtype=torch.int32, device=dev)
    rotation = torch.empty((nimg,), dtype=torch.float32, device=dev)
    reflection = torch.empty((nimg,), dtype=torch.float32, device=dev) if ref_table is not None else None
    with torch.cuda.device(dev), _timed("window_sums_tail"):
        st = lib.eqa_window_sums_tail(part.data_ptr(), weff.data_ptr(), act.data_ptr(), gidx.data_ptr(), rot_table.data_ptr(),
                                      ref_table.data_ptr() if ref_table is not None else None, rotation.data_ptr(),
                                      reflection.data_ptr() if reflection is not None else None, nimg, C, k, nseg, sub, E, float(scale),
                                      float(shift), _stream())
    _lib.check(st, "eqa_window_sums_tail")
    return act, gidx, rotation, reflection


def window_sums_gemv_bwd(dact: torch.Tensor, weff: torch.Tensor, S: torch.Tensor, scale: float, need_dS: bool, need_dW: bool):
    """Backward of `window_sums_gemv`: (dS (B,K) fp64 or None, dweff (E,K) fp64 or None) (eqa_window_sums_gemv_bwd)."""
    lib = _lib.load()
    dact = _need(dact, "dact")
    weff, S = _need(weff, "weff", torch.float64), _need(S, "S", torch.float64)
    B, K = S.shape
    E = weff.shape[0]
    dS = torch.empty_like(S) if need_dS else None
    dW = torch.empty_like(weff) if need_dW else None
    ws = torch.empty((max(lib.eqa_window_sums_gemv_bwd_workspace_bytes(K, E), 8) // 8,), dtype=torch.float64, device=S.device) if need_dW else None
    with torch.cuda.device(S.device), _timed("sums_gemv_bwd"):
        st = lib.eqa_window_sums_gemv_bwd(dact.data_ptr(), weff.data_ptr(), S.data_ptr(), dS.data_ptr() if need_dS else None,
                                          dW.data_ptr() if need_dW else None, ws.data_ptr() if need_dW else None, B, K, E, float(scale), _stream())
    _lib.check(st, "eqa_window_sums_gemv_bwd")
    return dS, dW


def window_grad_table(dS: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Backward of the window sums as a class table: dS (B,C,k,k) fp64 -> (B, 2k-1, 2k-1, C) fp32 (eqa_window_grad_table)."""
    lib = _lib.load()
    dS = _need(dS, "dS", torch.float64)
    B, C, k, _ = dS.shape
    T = 2 * (k - 1) + 1
    table = torch.empty((B, T, T, C), dtype=torch.float32, device=dS.device)
    with torch.cuda.device(dS.device), _timed("window_grad_table"):
        st = lib.eqa_window_grad_table(dS.data_ptr(), table.data_ptr(), B, C, H, W, k, _stream())
    _lib.check(st, "eqa_window_grad_table")
    return table


def plane_gemm_supported(cin: int, cout: int) -> bool:
    return bool(_lib.load().eqa_plane_gemm_supported(cin, cout))


def pack_plane_gemm_weights(U: torch.Tensor) -> torch.Tensor:
    """(P, Cin, Cout) Winograd-domain filters -> the MFMA operand-fragment order of eqa_plane_gemm:
    Upk[p][s][n][b][32 h + i][t] = U[p][16 s + 8 b + 4 h + t][32 n + i]."""
    P, Cin, Cout = U.shape
    t = U.float().reshape(P, Cin // 16, 2, 2, 4, Cout // 32, 32)        # p, s, b, h, t, n, i
    return t.permute(0, 1, 5, 2, 3, 6, 4).contiguous()                   # p, s, n, b, h, i, t


def plane_gemm(V: torch.Tensor, Upk: torch.Tensor, M: torch.Tensor, tiles: int) -> None:
    """M[:tiles, a] = V[:tiles, a] . U[a] for every plane a (eqa_plane_gemm); V:(T,P,Cin), M:(T,P,Cout) contiguous."""
    lib = _lib.load()
    V, Upk, M = _need(V, "V"), _need(Upk, "Upk"), _need(M, "M")
    P, Cin = V.shape[1], V.shape[2]
    Cout = M.shape[2]
    with torch.cuda.device(V.device):
        st = lib.eqa_plane_gemm(V.data_ptr(), Upk.data_ptr(), M.data_ptr(), tiles, P, Cin, Cout, _stream())
    _lib.check(st, "eqa_plane_gemm")


def lift_conv_supported(cin: int, kh: int, kw: int, cout: int) -> bool:
    """Shapes eqa_lift_conv_nhwc takes (others: the framework's convolution)."""
    return kh in (3, 5) and 9 <= kw * cin <= 15 and cout % 16 == 0


def pack_lift_weights(bank: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, KH, KW) filters -> (KH*8, 2, Cout) operand of eqa_lift_conv_nhwc (layout: include/eqa_hip.h): every
    filter row of R = KW*Cin floats is split into two 8-element halves starting at 0 and R-8; the elements the halves
    share get weight 0 in the second one."""
    Cout, Cin, KH, KW = bank.shape
    R = KW * Cin
    rows = bank.permute(2, 3, 1, 0).reshape(KH, R, Cout)                # [ky][j = kx*Cin + ci][co]
    q = torch.arange(8, device=bank.device)
    first = rows[:, q]                                                  # (KH, 8, Cout)
    second = rows[:, (R - 8) + q].clone()
    second[:, : 16 - R] = 0
    return torch.stack([first, second], dim=2).reshape(KH * 8, 2, Cout).float().contiguous()


def lift_conv_nhwc(x: torch.Tensor, wpk: torch.Tensor, bias: Optional[torch.Tensor], relu: bool, kh: int, kw: int) -> torch.Tensor:
    """Channels-last (B,Cin,H,W) -> channels-last (B,Cout,H-kh+1,W-kw+1) = [relu](conv2d(x, w) + bias) on the fp32 MFMA
    (eqa_lift_conv_nhwc); wpk = pack_lift_weights(w)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("lift_conv_nhwc expects a channels-last fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    bias, p_bias = _opt(bias, "bias", torch.float32)
    B, Cin, H, W = x.shape
    Cout = wpk.shape[2]
    y = torch.empty((B, Cout, H - kh + 1, W - kw + 1), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device), _timed("lift_conv"):
        st = lib.eqa_lift_conv_nhwc(x.data_ptr(), wpk.data_ptr(), p_bias, int(relu), y.data_ptr(), B, H, W, Cin, kh, kw, Cout, _stream())
    _lib.check(st, "eqa_lift_conv_nhwc")
    return y


def lift_conv_wide_supported(cin: int, kh: int, kw: int, cout: int) -> bool:
    """Shapes eqa_lift_conv_wide takes: the lifting filters eqa_lift_conv_nhwc does not (7 x 7 / 9 x 9 over RGB, 3 ... 9 over one channel)."""
    return bool(_lib.load().eqa_lift_conv_wide_supported(cin, kh, kw, cout))


def pack_lift_weights_wide(bank: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, KH, KW) filters -> (Cout/64, (R+1)/2, 2, 64) operand of eqa_lift_conv_wide (layout: include/eqa_hip.h): tap
    r = (ky*KW + kx)*Cin + ci, two taps per matrix instruction, a zero tap where R is odd."""
    Cout, Cin, KH, KW = bank.shape
    R = KH * KW * Cin
    steps = (R + 1) // 2
    taps = bank.permute(0, 2, 3, 1).reshape(Cout, R).float()            # [co][r]
    if 2 * steps > R:
        taps = torch.cat([taps, taps.new_zeros(Cout, 2 * steps - R)], dim=1)
    # [slice][nt][c32][step][khalf] -> [slice][step][nt][khalf][c32]
    t = taps.view(Cout // 64, 2, 32, steps, 2).permute(0, 3, 1, 4, 2)
    return t.reshape(Cout // 64, steps, 2, 64).contiguous()


def lift_conv_wide(x: torch.Tensor, wpk: torch.Tensor, bias: Optional[torch.Tensor], relu: bool, kh: int, kw: int) -> torch.Tensor:
    """`lift_conv_nhwc` for the wide / single-channel lifting filters (eqa_lift_conv_wide); wpk = pack_lift_weights_wide(w)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("lift_conv_wide expects a channels-last fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    bias, p_bias = _opt(bias, "bias", torch.float32)
    B, Cin, H, W = x.shape
    Cout = wpk.shape[0] * 64
    y = torch.empty((B, Cout, H - kh + 1, W - kw + 1), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device), _timed("lift_conv"):
        st = lib.eqa_lift_conv_wide(x.data_ptr(), wpk.data_ptr(), p_bias, int(relu), y.data_ptr(), B, H, W, Cin, kh, kw, Cout, _stream())
    _lib.check(st, "eqa_lift_conv_wide")
    return y


def lift_conv_wide_wgrad(x: torch.Tensor, dy: torch.Tensor, kh: int, kw: int) -> torch.Tensor:
    """d loss / d filters (Cout, Cin, kh, kw) of `lift_conv_wide` from channels-last x and dy, deterministic (eqa_lift_conv_wide_wgrad)."""
    lib = _lib.load()
    for t, name in ((x, "x"), (dy, "dy")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError(f"lift_conv_wide_wgrad expects a channels-last fp32 tensor on the device for {name}")
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    if tuple(dy.shape) != (B, Cout, H - kh + 1, W - kw + 1):
        raise RuntimeError("lift_conv_wide_wgrad: dy does not match x and the kernel size")
    ws = torch.empty(max(lib.eqa_lift_conv_wide_wgrad_workspace_bytes(Cin, kh, kw, Cout), 16) // 4, dtype=torch.float32, device=x.device)
    dbank = torch.empty((Cout, Cin, kh, kw), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.eqa_lift_conv_wide_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dbank.data_ptr(), B, H, W, Cin, kh, kw, Cout, _stream())
    _lib.check(st, "eqa_lift_conv_wide_wgrad")
    return dbank


def lift_conv_stats_supported(x_shape, kh: int, kw: int, cout: int) -> bool:
    """Shapes eqa_lift_conv_nhwc_stats takes (x_shape: (B, Cin, H, W))."""
    B, Cin, H, W = x_shape
    return _lib.load().eqa_lift_conv_stats_rows(B, H, W, Cin, kh, kw, cout) > 0


def lift_conv_nhwc_stats(x: torch.Tensor, wpk: torch.Tensor, kh: int, kw: int):
    """`lift_conv_nhwc` without bias / activation that also returns the fp64 partial sums (rows, Cout, 2) of the output's
    per-channel sum and sum of squares (eqa_lift_conv_nhwc_stats) -- what the batch-norm behind the lifting layer needs, taken
    from the values on their way out of the kernel.  None as the second result: this shape has no such form."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("lift_conv_nhwc_stats expects a channels-last fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    B, Cin, H, W = x.shape
    Cout = wpk.shape[2]
    rows = lib.eqa_lift_conv_stats_rows(B, H, W, Cin, kh, kw, Cout)
    if rows <= 0:
        return lift_conv_nhwc(x, wpk, None, False, kh, kw), None
    y = torch.empty((B, Cout, H - kh + 1, W - kw + 1), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    part = torch.empty((rows, Cout, 2), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device), _timed("lift_conv"):
        st = lib.eqa_lift_conv_nhwc_stats(x.data_ptr(), wpk.data_ptr(), y.data_ptr(), part.data_ptr(), B, H, W, Cin, kh, kw, Cout, _stream())
    _lib.check(st, "eqa_lift_conv_nhwc_stats")
    return y, part


def lift_conv_grouped(x: torch.Tensor, wpk: torch.Tensor, bias: Optional[torch.Tensor], relu: bool, kh: int, kw: int) -> torch.Tensor:
    """`lift_conv_nhwc` with the output in the channel-group-major layout (B, Cout/16, H-kh+1, W-kw+1, 16) that the FFT
    convolution's input transform reads in whole cache lines (eqa_lift_conv_grouped)."""
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("lift_conv_grouped expects a channels-last fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    bias, p_bias = _opt(bias, "bias", torch.float32)
    B, Cin, H, W = x.shape
    Cout = wpk.shape[2]
    y = torch.empty((B, Cout // 16, H - kh + 1, W - kw + 1, 16), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("lift_conv"):
        st = lib.eqa_lift_conv_grouped(x.data_ptr(), wpk.data_ptr(), p_bias, int(relu), y.data_ptr(), B, H, W, Cin, kh, kw, Cout, _stream())
    _lib.check(st, "eqa_lift_conv_grouped")
    return y


def lift_conv_wgrad_supported(x: torch.Tensor, cout: int, kh: int, kw: int) -> bool:
    """Shapes eqa_lift_conv_wgrad_nhwc takes (others: the framework's convolution-weight-gradient)."""
    B, Cin, H, W = x.shape
    return bool(_lib.load().eqa_lift_conv_wgrad_supported(B, H, W, Cin, cout, kh, kw))


def lift_conv_wgrad_nhwc(x: torch.Tensor, dy: torch.Tensor, kh: int, kw: int) -> torch.Tensor:
    """d loss / d filters (Cout, Cin, kh, kw) of y = conv2d(x, w) from channels-last x (B,Cin,H,W) and dy (B,Cout,H-kh+1,W-kw+1)
    on the fp32 MFMA, deterministic (eqa_lift_conv_wgrad_nhwc)."""
    lib = _lib.load()
    for t, name in ((x, "x"), (dy, "dy")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError(f"lift_conv_wgrad_nhwc expects a channels-last fp32 tensor on the device for {name}")
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    if tuple(dy.shape) != (B, Cout, H - kh + 1, W - kw + 1):
        raise RuntimeError("lift_conv_wgrad_nhwc: dy does not match x and the kernel size")
    ws = torch.empty(max(lib.eqa_lift_conv_wgrad_workspace_bytes(B, H, W, Cin, Cout, kh, kw), 16) // 4, dtype=torch.float32, device=x.device)
    dbank = torch.empty((Cout, Cin, kh, kw), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.eqa_lift_conv_wgrad_nhwc(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dbank.data_ptr(), B, H, W, Cin, Cout, kh, kw, _stream())
    _lib.check(st, "eqa_lift_conv_wgrad_nhwc")
    return dbank


def image_action_nearest(x: torch.Tensor, eidx: torch.Tensor, rtheta: torch.Tensor, flags: Optional[torch.Tensor],
                         pad: int, out_hw: Tuple[int, int], top_left: Tuple[int, int], n_planes: int, src_mod: int) -> torch.Tensor:
    """fp32 planes (P,H,W) -> (n_planes, OH, OW): nearest-neighbour action with edge pad + crop (eqa_image_action_nearest)."""
    lib = _lib.load()
    x = _need(x, "x")
    eidx = _need(eidx, "eidx", torch.int32)
    rtheta = _need(rtheta, "rtheta")
    flags, p_flags = _opt(flags, "flags", torch.int32)
    P, H, W = x.shape
    out = torch.empty((n_planes, out_hw[0], out_hw[1]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.eqa_image_action_nearest(x.data_ptr(), out.data_ptr(), eidx.data_ptr(), rtheta.data_ptr(), p_flags,
                                          rtheta.shape[0], n_planes, src_mod, H, W, pad, out_hw[0], out_hw[1],
                                          top_left[0], top_left[1], _stream())
    _lib.check(st, "eqa_image_action_nearest")
    return out


def gram_schmidt_backward(v: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """dL/dv of `gram_schmidt` from dL/d(out), both (B,3,3) (eqa_gram_schmidt_bwd)."""
    lib = _lib.load()
    v = _need(v, "vectors")
    grad_out = _need(grad_out, "grad_out")
    if v.dim() != 3 or v.shape[1:] != (3, 3) or grad_out.shape != v.shape:
        raise ValueError("gram_schmidt_backward expects two (B,3,3) tensors")
    gv = torch.empty_like(v)
    with torch.cuda.device(v.device):
        st = lib.eqa_gram_schmidt_bwd(v.data_ptr(), grad_out.data_ptr(), gv.data_ptr(), v.shape[0], _stream())
    _lib.check(st, "eqa_gram_schmidt_bwd")
    return gv


def modified_gram_schmidt(v: torch.Tensor) -> torch.Tensor:
    """(B,3,3) -> orthonormal rows by MODIFIED Gram-Schmidt (n-body canonicalizer; eqa_modified_gram_schmidt)."""
    lib = _lib.load()
    v = _need(v, "vectors")
    out = torch.empty_like(v)
    with torch.cuda.device(v.device):
        st = lib.eqa_modified_gram_schmidt(v.data_ptr(), out.data_ptr(), v.shape[0], _stream())
    _lib.check(st, "eqa_modified_gram_schmidt")
    return out


def rigid_rows(x: torch.Tensor, R: torch.Tensor, t: Optional[torch.Tensor], inverse: bool) -> torch.Tensor:
    """Per-row rigid action on (M,3) row vectors: x R + t (inverse=False) or x R^T - t R^T (inverse=True)."""
    lib = _lib.load()
    x = _need(x, "x")
    R = _need(R, "R")
    t, p_t = _opt(t, "t", torch.float32)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = lib.eqa_rigid_rows(x.data_ptr(), R.data_ptr(), p_t, out.data_ptr(), x.shape[0], int(inverse), _stream())
    _lib.check(st, "eqa_rigid_rows")
    return out


def _rows(what: str, M: Optional[int], **named) -> int:
    """Every given tensor is (M, *tail): named as name=(tensor or None, tail); returns M.  Shapes are judged before anything else, so
    a wrong one is a ValueError whatever device it is on."""
    for name, (t, tail) in named.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or (M is not None and t.shape[0] != M):
            want = ",".join(str(d) for d in ("M" if M is None else M,) + tail)
            raise ValueError(f"{what}: {name} must be ({want}), got {tuple(t.shape)}")
        M = t.shape[0]
    return M


def nbody_frame_fwd(v: torch.Tensor, t: torch.Tensor, loc: torch.Tensor, vel: torch.Tensor
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The n-body canonicalizer's forward in one launch: v:(M,3,3), t, loc, vel:(M,3) -> (R, cloc, cvel), the bits of
    `modified_gram_schmidt` followed by `rigid_rows(loc, R, t, inverse=True)` and `rigid_rows(vel, R, None, inverse=True)`
    (eqa_nbody_frame_fwd)."""
    for name, x in (("vectors", v), ("t", t), ("loc", loc), ("vel", vel)):
        if x is None:
            raise TypeError(f"{name} must be a torch.Tensor")
    M = _rows("nbody_frame_fwd", None, vectors=(v, (3, 3)), t=(t, (3,)), loc=(loc, (3,)), vel=(vel, (3,)))
    lib = _lib.load()
    v, t, loc, vel = _need(v, "vectors"), _need(t, "t"), _need(loc, "loc"), _need(vel, "vel")
    R, cloc, cvel = torch.empty_like(v), torch.empty_like(loc), torch.empty_like(vel)
    with torch.cuda.device(v.device):
        st = lib.eqa_nbody_frame_fwd(v.data_ptr(), t.data_ptr(), loc.data_ptr(), vel.data_ptr(), R.data_ptr(), cloc.data_ptr(),
                                     cvel.data_ptr(), M, _stream())
    _lib.check(st, "eqa_nbody_frame_fwd")
    return R, cloc, cvel


def nbody_frame_bwd(v: torch.Tensor, t: Optional[torch.Tensor], loc: Optional[torch.Tensor], vel: Optional[torch.Tensor],
                    R: Optional[torch.Tensor], gR: Optional[torch.Tensor], gcloc: Optional[torch.Tensor],
                    gcvel: Optional[torch.Tensor], need: Tuple[bool, bool, bool, bool] = (True, True, True, True)
                    ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Backward of `nbody_frame_fwd` in one launch (eqa_nbody_frame_bwd): incoming gR:(M,3,3), gcloc, gcvel:(M,3), each None for
    zero -> (gv, gt, gloc, gvel), None where ``need`` says not wanted.  With gcloc = gcvel = None and need = (True, False, False,
    False) it is the backward of `modified_gram_schmidt`, and t, loc, vel, R may be None."""
    if v is None:
        raise TypeError("vectors must be a torch.Tensor")
    M = _rows("nbody_frame_bwd", None, vectors=(v, (3, 3)), t=(t, (3,)), loc=(loc, (3,)), vel=(vel, (3,)), R=(R, (3, 3)),
              gR=(gR, (3, 3)), gcloc=(gcloc, (3,)), gcvel=(gcvel, (3,)))
    need_v, need_t, need_loc, need_vel = (bool(n) for n in need)
    if not (need_v or need_t or need_loc or need_vel):
        raise ValueError("nbody_frame_bwd: no gradient wanted")
    if (need_t or need_loc or need_vel) and R is None:
        raise ValueError("nbody_frame_bwd: gt, gloc and gvel need the frame R the forward returned")
    if need_v and ((gcloc is not None and (loc is None or t is None)) or (gcvel is not None and vel is None)):
        raise ValueError("nbody_frame_bwd: gv needs loc and t with gcloc, vel with gcvel")
    lib = _lib.load()
    v = _need(v, "vectors")
    t, p_t = _opt(t, "t", torch.float32)
    loc, p_loc = _opt(loc, "loc", torch.float32)
    vel, p_vel = _opt(vel, "vel", torch.float32)
    R, p_R = _opt(R, "R", torch.float32)
    gR, p_gR = _opt(gR, "gR", torch.float32)
    gcloc, p_gcloc = _opt(gcloc, "gcloc", torch.float32)
    gcvel, p_gcvel = _opt(gcvel, "gcvel", torch.float32)
    new = lambda shape: torch.empty(shape, dtype=torch.float32, device=v.device)      # noqa: E731
    gv = new((M, 3, 3)) if need_v else None
    gt, gloc, gvel = (new((M, 3)) if n else None for n in (need_t, need_loc, need_vel))
    ptr = lambda x: None if x is None else x.data_ptr()                               # noqa: E731
    with torch.cuda.device(v.device):
        st = lib.eqa_nbody_frame_bwd(v.data_ptr(), p_t, p_loc, p_vel, p_R, p_gR, p_gcloc, p_gcvel, ptr(gv), ptr(gt), ptr(gloc),
                                     ptr(gvel), M, _stream())
    _lib.check(st, "eqa_nbody_frame_bwd")
    return gv, gt, gloc, gvel


def rigid_rows_bwd(x: Optional[torch.Tensor], R: Optional[torch.Tensor], g: torch.Tensor, need: Tuple[bool, bool] = (True, True)
                   ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Backward of `rigid_rows(x, R, t, inverse=False)` (eqa_rigid_rows_bwd): g:(M,3) -> (gx = g R^T, gR[i][j] = x_i g_j), None
    where ``need`` says not wanted.  The gradient of t is g itself."""
    if g is None:
        raise TypeError("g must be a torch.Tensor")
    M = _rows("rigid_rows_bwd", None, g=(g, (3,)), x=(x, (3,)), R=(R, (3, 3)))
    need_x, need_R = bool(need[0]), bool(need[1])
    if not (need_x or need_R) or (need_x and R is None) or (need_R and x is None):
        raise ValueError("rigid_rows_bwd: gx needs R, gR needs x, and one of the two must be wanted")
    lib = _lib.load()
    g = _need(g, "g")
    x, p_x = _opt(x, "x", torch.float32)
    R, p_R = _opt(R, "R", torch.float32)
    gx = torch.empty_like(g) if need_x else None
    gR = torch.empty((M, 3, 3), dtype=torch.float32, device=g.device) if need_R else None
    with torch.cuda.device(g.device):
        st = lib.eqa_rigid_rows_bwd(p_x, p_R, g.data_ptr(), None if gx is None else gx.data_ptr(),
                                    None if gR is None else gR.data_ptr(), M, _stream())
    _lib.check(st, "eqa_rigid_rows_bwd")
    return gx, gR


FOURIER_FIELD_DIM = 9  # channels of a band-limited SO(2) field: a_0, (Re, Im) c_1..c_4 (csrc/fourier_act.hip)


def _fourier_args(x: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], what: str):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError(f"{what} expects a channels-last fp32 (B, 9 * fields, H, W) tensor on the device")
    B, C, H, W = x.shape
    if C == 0 or C % FOURIER_FIELD_DIM:
        raise ValueError(f"{what}: {C} channels are not a whole number of 9-channel fields")
    fields = C // FOURIER_FIELD_DIM
    scale, p_scale = _opt(scale, "scale", torch.float32)
    shift, p_shift = _opt(shift, "shift", torch.float32)
    if scale is not None and tuple(scale.shape) != (fields, 5):
        raise ValueError(f"{what}: scale must be (fields, 5) = ({fields}, 5), got {tuple(scale.shape)}")
    if shift is not None and tuple(shift.shape) != (fields,):
        raise ValueError(f"{what}: shift must be (fields,) = ({fields},), got {tuple(shift.shape)}")
    return B * H * W, fields, (scale, shift), p_scale, p_shift


def fourier_elu(x: torch.Tensor, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FourierELU (16 samples, frequencies 0..4) of scale * x + shift on a channels-last (B, 9 * fields, H, W) map, one pass
    (eqa_fourier_elu_fwd).  scale:(fields, 5) per field and frequency, shift:(fields,) on a_0; None: ones / zeros."""
    lib = _lib.load()
    npix, fields, keep, p_scale, p_shift = _fourier_args(x, scale, shift, "fourier_elu")
    y = torch.empty_like(x)
    if npix == 0:
        return y
    with torch.cuda.device(x.device), _timed("fourier_elu"):
        st = lib.eqa_fourier_elu_fwd(x.data_ptr(), p_scale, p_shift, y.data_ptr(), npix, fields, _stream())
    _lib.check(st, "eqa_fourier_elu_fwd")
    return y


def fourier_elu_bwd(x: torch.Tensor, dy: torch.Tensor, scale: Optional[torch.Tensor] = None,
                    shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d/dx of `fourier_elu` (eqa_fourier_elu_bwd): the samples are recomputed from x, the scale is applied inside."""
    lib = _lib.load()
    npix, fields, keep, p_scale, p_shift = _fourier_args(x, scale, shift, "fourier_elu_bwd")
    if not (isinstance(dy, torch.Tensor) and dy.is_cuda and dy.dtype == torch.float32 and dy.shape == x.shape
            and dy.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError("fourier_elu_bwd expects dy channels-last fp32 on the device, shaped like x")
    dx = torch.empty_like(x)
    if npix == 0:
        return dx
    with torch.cuda.device(x.device), _timed("fourier_elu_bwd"):
        st = lib.eqa_fourier_elu_bwd(x.data_ptr(), p_scale, p_shift, dy.data_ptr(), dx.data_ptr(), npix, fields, _stream())
    _lib.check(st, "eqa_fourier_elu_bwd")
    return dx


FIELD_NORM_MAX_FIELDS = 64   # == eqa_field_norm_max_fields() (csrc/field_norm.hip: one field per thread for a block's whole walk)


def _field_norm_args(x: torch.Tensor, dy: Optional[torch.Tensor], scale, shift, what: str):
    """`_fourier_args`, the field limit of the training kernels, dy shaped and laid out like x, and the rows of `partial`."""
    npix, fields, keep, p_scale, p_shift = _fourier_args(x, scale, shift, what)
    if fields > FIELD_NORM_MAX_FIELDS:
        raise _lib.EqaLibraryError(f"{what}: {fields} fields, the field-norm kernels take at most {FIELD_NORM_MAX_FIELDS}")
    if dy is not None and not (isinstance(dy, torch.Tensor) and dy.is_cuda and dy.dtype == torch.float32 and dy.shape == x.shape
                               and dy.is_contiguous(memory_format=torch.channels_last)):
        raise RuntimeError(f"{what} expects dy channels-last fp32 on the device, shaped like x")
    blocks = int(_lib.load().eqa_field_norm_blocks(npix, fields)) if npix else 0
    if npix and blocks <= 0:
        _lib.check(blocks, "eqa_field_norm_blocks")
    return npix, fields, keep, p_scale, p_shift, blocks


def field_norm_stats(x: torch.Tensor) -> torch.Tensor:
    """partial:(blocks, fields, 6) fp64 of a channels-last (B, 9 * fields, H, W) map (eqa_field_norm_stats): per block of the walk
    and field sum a_0, sum a_0^2, sum (Re^2 + Im^2) of c_1..c_4.  ``partial.sum(0)`` are the sums over the map."""
    lib = _lib.load()
    npix, fields, _, _, _, blocks = _field_norm_args(x, None, None, None, "field_norm_stats")
    partial = torch.empty((blocks, fields, 6), dtype=torch.float64, device=x.device)
    if npix == 0:
        return partial
    with torch.cuda.device(x.device), _timed("field_norm_stats"):
        st = lib.eqa_field_norm_stats(x.data_ptr(), partial.data_ptr(), npix, fields, _stream())
    _lib.check(st, "eqa_field_norm_stats")
    return partial


def field_norm_elu_bwd_reduce(x: torch.Tensor, dy: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """partial:(blocks, fields, 6) fp64 (eqa_field_norm_elu_bwd_reduce): with du the gradient of `fourier_elu(x, scale, shift)` at
    u = scale x + shift, per block and field sum du_0, sum du_0 a_0, sum (du_Re Re + du_Im Im) of c_1..c_4."""
    lib = _lib.load()
    npix, fields, keep, p_scale, p_shift, blocks = _field_norm_args(x, dy, scale, shift, "field_norm_elu_bwd_reduce")
    partial = torch.empty((blocks, fields, 6), dtype=torch.float64, device=x.device)
    if npix == 0:
        return partial
    with torch.cuda.device(x.device), _timed("field_norm_elu_bwd_reduce"):
        st = lib.eqa_field_norm_elu_bwd_reduce(x.data_ptr(), p_scale, p_shift, dy.data_ptr(), partial.data_ptr(), npix, fields, _stream())
    _lib.check(st, "eqa_field_norm_elu_bwd_reduce")
    return partial


def field_norm_elu_bwd_apply(x: torch.Tensor, dy: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor,
                             coef: torch.Tensor) -> torch.Tensor:
    """dx of the training-mode field norm + FourierELU (eqa_field_norm_elu_bwd_apply).  coef:(fields, 7) = (k_0, mean, c_1..c_5):
    dx_0 = scale_0 du_0 - k_0 - c_1 (a_0 - mean), dx_j = scale_m du_j - c_{1+m} x_j; du is formed again from x and dy."""
    lib = _lib.load()
    npix, fields, keep, p_scale, p_shift, _ = _field_norm_args(x, dy, scale, shift, "field_norm_elu_bwd_apply")
    coef = _need(coef, "coef")
    if tuple(coef.shape) != (fields, 7):
        raise ValueError(f"field_norm_elu_bwd_apply: coef must be (fields, 7) = ({fields}, 7), got {tuple(coef.shape)}")
    dx = torch.empty_like(x)
    if npix == 0:
        return dx
    with torch.cuda.device(x.device), _timed("field_norm_elu_bwd_apply"):
        st = lib.eqa_field_norm_elu_bwd_apply(x.data_ptr(), p_scale, p_shift, dy.data_ptr(), coef.data_ptr(), dx.data_ptr(), npix,
                                              fields, _stream())
    _lib.check(st, "eqa_field_norm_elu_bwd_apply")
    return dx


def steer_lift_supported(cin: int, k: int, fields: int) -> bool:
    """Shapes the steerable lifting kernels take (eqa_steer_lift_supported): 1 or 3 input channels, k in {5, 7, 9}, 1..64 fields."""
    return bool(_lib.load().eqa_steer_lift_supported(cin, k, fields))


def steer_lift_layout(cin: int, k: int, fields: int) -> Tuple[int, int, int, int]:
    """(groups, blocks per wave, steps, padded filter-row floats) of the packed operand (csrc/steer_lift.hip, file header): the
    ceil(9 fields / 16) 16-channel blocks in groups of at most 3; a filter row of k cin floats padded to whole 4-tap steps."""
    nblk = (FOURIER_FIELD_DIM * fields + 15) // 16
    groups = (nblk + 2) // 3
    rwp = (k * cin + 3) // 4 * 4
    return groups, (nblk + groups - 1) // groups, k * (rwp // 4), rwp


def pack_steer_lift_weights(bank: torch.Tensor) -> torch.Tensor:
    """(9 fields, Cin, K, K) bank -> (groups, bpw, steps, 64) operand of eqa_steer_lift_fwd, in torch ops on the bank's device:
    wpk[g][b][s][lane] = bank[16 (g bpw + b) + (lane & 15)][ci][ky][kx] with ky = s // (rwp/4), column 4 (s % (rwp/4)) + (lane >> 4)
    = kx Cin + ci; zero for the columns past K Cin and the channels past 9 fields."""
    C9, Cin, K, K2 = bank.shape
    if K != K2 or C9 % FOURIER_FIELD_DIM:
        raise ValueError(f"pack_steer_lift_weights: a (9 fields, Cin, K, K) bank is expected, got {tuple(bank.shape)}")
    groups, bpw, steps, rwp = steer_lift_layout(Cin, K, C9 // FOURIER_FIELD_DIM)
    rows = bank.detach().float().permute(0, 2, 3, 1).reshape(C9, K, K * Cin)       # [co][ky][kx Cin + ci]
    padded = rows.new_zeros(groups * bpw * 16, K, rwp)
    padded[:C9, :, :K * Cin] = rows
    # [g][b][li][ky][cs][q] -> [g][b][ky][cs][q][li]
    t = padded.view(groups, bpw, 16, K, rwp // 4, 4).permute(0, 1, 3, 4, 5, 2)
    return t.reshape(groups, bpw, steps, 64).contiguous()


def _steer_lift_map(t: torch.Tensor, name: str, what: str) -> torch.Tensor:
    """t as the kernels read it: fp32, on the device, channels-last (for one channel a contiguous NCHW map is the same memory)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise RuntimeError(f"{what} expects {name} as a 4-d fp32 tensor on the device")
    if not (t.is_contiguous(memory_format=torch.channels_last) or (t.shape[1] == 1 and t.is_contiguous())):
        raise RuntimeError(f"{what} expects {name} channels-last")
    return t


def steer_lift(x: torch.Tensor, wpk: torch.Tensor, k: int, fields: int, with_stats: bool = False):
    """y:(B, 9 fields, H-k+1, W-k+1) channels-last = conv2d(x, bank) for wpk = pack_steer_lift_weights(bank) (eqa_steer_lift_fwd).
    with_stats: also the (fields, 6) fp64 sums of `field_norm_stats(y).sum(0)` (sum a_0, sum a_0^2, sum (Re^2 + Im^2) of
    c_1..c_4), taken from the values on their way out of the kernel and folded here in torch ops on the device; else None."""
    lib = _lib.load()
    x = _steer_lift_map(x, "x", "steer_lift")
    wpk = _need(wpk, "wpk")
    B, Cin, H, W = x.shape
    if not steer_lift_supported(Cin, k, fields) or H < k or W < k:
        raise _lib.EqaLibraryError(f"steer_lift: (Cin, k, fields, H, W) = {(Cin, k, fields, H, W)} is not a shape the kernel takes")
    if wpk.numel() != lib.eqa_steer_lift_packed_floats(Cin, k, fields):
        raise ValueError("steer_lift: wpk is not pack_steer_lift_weights of a bank of this shape")
    C9 = FOURIER_FIELD_DIM * fields
    y = torch.empty((B, C9, H - k + 1, W - k + 1), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    part = torch.empty((int(lib.eqa_steer_lift_stat_rows(fields)), C9, 2), dtype=torch.float64, device=x.device) if with_stats else None
    if B == 0:
        return y, (torch.zeros((fields, 6), dtype=torch.float64, device=x.device) if with_stats else None)
    with torch.cuda.device(x.device), _timed("steer_lift"):
        st = lib.eqa_steer_lift_fwd(x.data_ptr(), wpk.data_ptr(), y.data_ptr(), part.data_ptr() if with_stats else None, B, H, W, Cin,
                                    k, fields, _stream())
    _lib.check(st, "eqa_steer_lift_fwd")
    if not with_stats:
        return y, None
    ch = part.sum(0).view(fields, FOURIER_FIELD_DIM, 2)                     # per channel: sum, sum of squares
    sq = ch[:, 1:, 1].reshape(fields, 4, 2).sum(2)                          # Re^2 + Im^2 of c_1..c_4
    return y, torch.cat([ch[:, 0, :], sq], dim=1)


def steer_lift_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int) -> torch.Tensor:
    """d loss / d bank (9 fields, Cin, k, k) of `steer_lift` from x and channels-last dy, deterministic (eqa_steer_lift_wgrad)."""
    lib = _lib.load()
    x = _steer_lift_map(x, "x", "steer_lift_wgrad")
    dy = _steer_lift_map(dy, "dy", "steer_lift_wgrad")
    B, Cin, H, W = x.shape
    C9 = dy.shape[1]
    fields = C9 // FOURIER_FIELD_DIM
    if C9 % FOURIER_FIELD_DIM or tuple(dy.shape) != (B, C9, H - k + 1, W - k + 1):
        raise RuntimeError("steer_lift_wgrad: dy does not match x and the kernel size")
    if not steer_lift_supported(Cin, k, fields):
        raise _lib.EqaLibraryError(f"steer_lift_wgrad: (Cin, k, fields) = {(Cin, k, fields)} is not a shape the kernel takes")
    if B == 0:
        return torch.zeros((C9, Cin, k, k), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(lib.eqa_steer_lift_wgrad_workspace_bytes(Cin, k, fields), 16) // 4, dtype=torch.float32, device=x.device)
    dbank = torch.empty((C9, Cin, k, k), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("steer_lift_wgrad"):
        st = lib.eqa_steer_lift_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dbank.data_ptr(), B, H, W, Cin, k, fields, _stream())
    _lib.check(st, "eqa_steer_lift_wgrad")
    return dbank


VNDEEPSETS_WIDTHS = (8, 16, 32)  # hidden widths the kernels are compiled for (csrc/nbody.hip); the caller zero-pads others
VNDEEPSETS_MAX_HIDDEN = 32
VNDEEPSETS_MAX_LAYERS = 8         # == kMaxLayers
NBODY_EDGES_OK = 4            # eqa_nbody_adjacency's flag when every edge stays inside a system and node M-1 has an incoming one


def nbody_adjacency(rows: torch.Tensor, cols: torch.Tensor, systems: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Edge list (rows = sources, cols = targets; int64) of `systems` 5-body systems -> (adj (systems, 5, 5) int32 in-edge counts
    [system][target][source], flag (1,) int32: NBODY_EDGES_OK iff the list suits the fused VNDeepSets kernels)."""
    lib = _lib.load()
    rows = _need(rows, "rows", torch.int64)
    cols = _need(cols, "cols", torch.int64)
    if rows.dim() != 1 or rows.shape != cols.shape or rows.numel() == 0:
        raise ValueError("nbody_adjacency expects two non-empty index vectors of one length")
    buf = torch.zeros(systems * 25 + 1, dtype=torch.int32, device=rows.device)      # one zero fill for the counts and the flag
    adj, flag = buf[:-1].view(systems, 5, 5), buf[-1:]
    with torch.cuda.device(rows.device), _timed("nbody_adjacency"):
        st = lib.eqa_nbody_adjacency(rows.data_ptr(), cols.data_ptr(), rows.numel(), systems, adj.data_ptr(), flag.data_ptr(), _stream())
    _lib.check(st, "eqa_nbody_adjacency")
    return adj, flag


def _vndeepsets_args(loc, vel, charges, adj, packed, hidden, layers, features):
    loc = _need(loc, "loc")
    M = loc.shape[0]
    if loc.dim() != 2 or loc.shape[1] != 3 or M == 0 or M % 5:
        raise ValueError(f"loc must be (5 * systems, 3), got {tuple(loc.shape)}")
    vel, p_vel = _opt(vel, "vel", torch.float32)
    charges, p_ch = _opt(charges, "charges", torch.float32)
    if vel is not None and tuple(vel.shape) != (M, 3):
        raise ValueError(f"vel must be ({M}, 3), got {tuple(vel.shape)}")
    if charges is not None and charges.numel() != M:
        raise ValueError(f"charges must hold one value per node ({M}), got {tuple(charges.shape)}")
    adj = _need(adj, "adj", torch.int32)
    if tuple(adj.shape) != (M // 5, 5, 5):
        raise ValueError(f"adj must be ({M // 5}, 5, 5), got {tuple(adj.shape)}")
    packed = _need(packed, "params")
    n = _lib.load().eqa_vndeepsets_param_count(hidden, layers, features)
    if packed.dim() != 1 or packed.numel() != n:
        raise ValueError(f"the packed parameters must be a vector of {n} values, got {tuple(packed.shape)}")
    return loc, vel, charges, adj, packed, p_vel, p_ch, M


def vndeepsets_fwd(loc, vel, charges, adj, packed, *, hidden, layers, features, softplus, slope, layer_mean, final_mean,
                   canon_translation) -> Tuple[torch.Tensor, torch.Tensor]:
    """VNDeepSets in one launch (eqa_vndeepsets_fwd): (rotation_vectors (M, 3, 3), translation_vectors (M, 3)).  No autograd."""
    lib = _lib.load()
    loc, vel, charges, adj, packed, p_vel, p_ch, M = _vndeepsets_args(loc, vel, charges, adj, packed, hidden, layers, features)
    rot = torch.empty(M, 3, 3, dtype=torch.float32, device=loc.device)
    trans = torch.empty(M, 3, dtype=torch.float32, device=loc.device)
    with torch.cuda.device(loc.device), _timed("vndeepsets_fwd"):
        st = lib.eqa_vndeepsets_fwd(loc.data_ptr(), p_vel, p_ch, adj.data_ptr(), packed.data_ptr(), rot.data_ptr(), trans.data_ptr(),
                                    M // 5, hidden, layers, features, int(softplus), slope, int(layer_mean), int(final_mean),
                                    int(canon_translation), _stream())
    _lib.check(st, "eqa_vndeepsets_fwd")
    return rot, trans


def vndeepsets_train_fwd(loc, vel, charges, adj, packed, mask, *, hidden, layers, features, softplus, slope, layer_mean, final_mean,
                         canon_translation) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """As `vndeepsets_fwd`, with dropout by the given factors mask:(layers, M, 3, hidden) (None: none); also returns the inputs of
    layers 1 .. layers-1, (layers - 1, M, 3, hidden), which `vndeepsets_bwd` needs."""
    lib = _lib.load()
    loc, vel, charges, adj, packed, p_vel, p_ch, M = _vndeepsets_args(loc, vel, charges, adj, packed, hidden, layers, features)
    mask, p_mask = _opt(mask, "mask", torch.float32)
    if mask is not None and tuple(mask.shape) != (layers, M, 3, hidden):
        raise ValueError(f"mask must be ({layers}, {M}, 3, {hidden}), got {tuple(mask.shape)}")
    rot = torch.empty(M, 3, 3, dtype=torch.float32, device=loc.device)
    trans = torch.empty(M, 3, dtype=torch.float32, device=loc.device)
    saved = torch.empty(layers - 1, M, 3, hidden, dtype=torch.float32, device=loc.device)
    with torch.cuda.device(loc.device), _timed("vndeepsets_train_fwd"):
        st = lib.eqa_vndeepsets_train_fwd(loc.data_ptr(), p_vel, p_ch, adj.data_ptr(), packed.data_ptr(), p_mask,
                                          saved.data_ptr() if layers > 1 else None, rot.data_ptr(), trans.data_ptr(), M // 5, hidden,
                                          layers, features, int(softplus), slope, int(layer_mean), int(final_mean),
                                          int(canon_translation), _stream())
    _lib.check(st, "eqa_vndeepsets_train_fwd")
    return rot, trans, saved


def vndeepsets_bwd(loc, vel, charges, adj, packed, mask, saved, grad_rot, grad_trans, *, hidden, layers, features, softplus, slope,
                   layer_mean, final_mean, canon_translation) -> torch.Tensor:
    """Per-block partial sums (blocks, n_params) of the packed parameters' gradient (eqa_vndeepsets_bwd); `.sum(0)` is the gradient."""
    lib = _lib.load()
    loc, vel, charges, adj, packed, p_vel, p_ch, M = _vndeepsets_args(loc, vel, charges, adj, packed, hidden, layers, features)
    mask, p_mask = _opt(mask, "mask", torch.float32)
    if mask is not None and tuple(mask.shape) != (layers, M, 3, hidden):
        raise ValueError(f"mask must be ({layers}, {M}, 3, {hidden}), got {tuple(mask.shape)}")
    saved = _need(saved, "saved")
    if tuple(saved.shape) != (layers - 1, M, 3, hidden):
        raise ValueError(f"saved must be ({layers - 1}, {M}, 3, {hidden}), got {tuple(saved.shape)}")
    grad_rot = _need(grad_rot, "grad_rot")
    grad_trans = _need(grad_trans, "grad_trans")
    if tuple(grad_rot.shape) != (M, 3, 3) or tuple(grad_trans.shape) != (M, 3):
        raise ValueError(f"grad_rot / grad_trans must be ({M}, 3, 3) / ({M}, 3), got {tuple(grad_rot.shape)} / {tuple(grad_trans.shape)}")
    blocks = lib.eqa_vndeepsets_bwd_blocks(M // 5)
    partial = torch.empty(blocks, packed.numel(), dtype=torch.float32, device=loc.device)
    with torch.cuda.device(loc.device), _timed("vndeepsets_bwd"):
        st = lib.eqa_vndeepsets_bwd(loc.data_ptr(), p_vel, p_ch, adj.data_ptr(), packed.data_ptr(), p_mask,
                                    saved.data_ptr() if layers > 1 else None, grad_rot.data_ptr(), grad_trans.data_ptr(),
                                    partial.data_ptr(), M // 5, hidden, layers, features, int(softplus), slope, int(layer_mean),
                                    int(final_mean), int(canon_translation), _stream())
    _lib.check(st, "eqa_vndeepsets_bwd")
    return partial


def _vn_act_args(x: torch.Tensor, Wd: torch.Tensor, what: str):
    x = _need(x, "x")
    Wd = _need(Wd, "Wd")
    if x.dim() < 3 or x.shape[2] != 3 or x.numel() == 0:
        raise ValueError(f"{what} expects a non-empty (B, C, 3, ...) tensor, got {tuple(x.shape)}")
    B, C = x.shape[0], x.shape[1]
    if Wd.dim() != 2 or Wd.shape[1] != C or Wd.shape[0] not in (1, C):
        raise ValueError(f"{what}: Wd must be ({C}, {C}) or (1, {C}), got {tuple(Wd.shape)}")
    return x, Wd, B, C, x.numel() // (B * C * 3), Wd.shape[0]


def vn_act_max_channels() -> int:
    """The widest layer the fused vector-neuron activation takes (eqa_vn_act_max_channels)."""
    return _lib.load().eqa_vn_act_max_channels()


def vn_act(x: torch.Tensor, Wd: torch.Tensor, softplus: bool, slope: float) -> torch.Tensor:
    """VNLeakyReLU (softplus False) or VNSoftplus of x:(B, C, 3, ...) with the direction map Wd:(C or 1, C), one pass
    (eqa_vn_act_fwd).  No autograd."""
    lib = _lib.load()
    x, Wd, B, C, P, D = _vn_act_args(x, Wd, "vn_act")
    y = torch.empty_like(x)
    with torch.cuda.device(x.device), _timed("vn_act"):
        st = lib.eqa_vn_act_fwd(x.data_ptr(), Wd.data_ptr(), y.data_ptr(), B, C, P, D, int(softplus), slope, _stream())
    _lib.check(st, "eqa_vn_act_fwd")
    return y


def vn_act_backward(x: torch.Tensor, Wd: torch.Tensor, gy: torch.Tensor, softplus: bool, slope: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dL/dx, dL/dWd) of `vn_act` for gy = dL/dy (eqa_vn_act_bwd); the per-block sums of dL/dWd are added here, in a fixed order."""
    lib = _lib.load()
    x, Wd, B, C, P, D = _vn_act_args(x, Wd, "vn_act_backward")
    gy = _need(gy, "gy")
    if gy.shape != x.shape:
        raise ValueError(f"gy must be shaped like x {tuple(x.shape)}, got {tuple(gy.shape)}")
    gx = torch.empty_like(x)
    partial = torch.empty(lib.eqa_vn_act_bwd_blocks(B * P), D, C, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("vn_act_bwd"):
        st = lib.eqa_vn_act_bwd(x.data_ptr(), Wd.data_ptr(), gy.data_ptr(), gx.data_ptr(), partial.data_ptr(), B, C, P, D,
                                int(softplus), slope, _stream())
    _lib.check(st, "eqa_vn_act_bwd")
    return gx, partial.sum(0)


def gconv1x1_supported(pixels: int, cin: int, cout: int) -> bool:
    """Shapes and sizes eqa_gconv1x1_nhwc takes: channel counts on the multiples of 32 from 32 to 512, every map inside one 32-bit
    buffer range (the size is part of the query: a caller that asks first takes its other route instead of failing in the launch)."""
    return bool(_lib.load().eqa_gconv1x1_supported(pixels, cin, cout))


def pack_gconv1x1_weights(bank: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin) or (Cout, Cin, 1, 1) filters of a 1 x 1 convolution -> the MFMA operand-fragment order of eqa_gconv1x1_nhwc:
    Wpk[s][n][b][32 h + i][t] = bank[32 n + i][16 s + 8 b + 4 h + t]  (`pack_plane_gemm_weights` of the one plane bank^T)."""
    Cout, Cin = bank.shape[:2]
    if bank.numel() != Cout * Cin:
        raise ValueError(f"pack_gconv1x1_weights takes the filters of a 1 x 1 convolution, got {tuple(bank.shape)}")
    return pack_plane_gemm_weights(bank.reshape(Cout, Cin).t()[None])[0]


def gconv1x1_nhwc(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, res: Optional[torch.Tensor] = None,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """y = act(conv1x1(x) + bias [+ res]), act(z) = [relu](scale[c] * z + shift[c]), one launch (eqa_gconv1x1_nhwc).  x: a
    channels-last (B, Cin, H, W) map or its (pixels, Cin) matrix; res and the result likewise with Cout channels;
    wpk = pack_gconv1x1_weights(filters); scale and shift together or not at all.  No autograd."""
    lib = _lib.load()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError("gconv1x1_nhwc expects an fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    Cin, Cout = wpk.shape[0] * 16, wpk.shape[1] * 32

    def rows(t, name, C):
        if t.dim() == 4:
            if t.shape[1] != C or not t.is_contiguous(memory_format=torch.channels_last):
                raise RuntimeError(f"gconv1x1_nhwc: {name} must be a channels-last map of {C} channels, got {tuple(t.shape)}")
            return t.shape[0] * t.shape[2] * t.shape[3]
        if t.dim() != 2 or t.shape[1] != C or not t.is_contiguous():
            raise RuntimeError(f"gconv1x1_nhwc: {name} must be a contiguous (pixels, {C}) matrix, got {tuple(t.shape)}")
        return t.shape[0]

    P = rows(x, "x", Cin)
    bias = _need(bias, "bias")
    if (scale is None) != (shift is None):
        raise ValueError("gconv1x1_nhwc: scale and shift come together")
    scale, p_scale = _opt(scale, "scale", torch.float32)
    shift, p_shift = _opt(shift, "shift", torch.float32)
    if any(v is not None and v.numel() != Cout for v in (bias, scale, shift)):
        raise ValueError(f"gconv1x1_nhwc: bias, scale and shift have {Cout} entries")
    p_res = None
    if res is not None:
        if res.dtype != torch.float32 or res.device != x.device or rows(res, "res", Cout) != P or res.dim() != x.dim():
            raise RuntimeError("gconv1x1_nhwc: res must be an fp32 map of the output's shape and layout on x's device")
        p_res = res.data_ptr()
    if not gconv1x1_supported(P, Cin, Cout):
        raise _lib.EqaLibraryError(f"eqa_gconv1x1_nhwc does not take {P} pixels of {Cin} -> {Cout} channels (ask gconv1x1_supported first)")
    if x.dim() == 4:
        y = torch.empty((x.shape[0], Cout, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    else:
        y = torch.empty((P, Cout), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("gconv1x1"):
        st = lib.eqa_gconv1x1_nhwc(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), p_res, p_scale, p_shift, int(relu), y.data_ptr(), P, Cin, Cout,
                                   _stream())
    _lib.check(st, "eqa_gconv1x1_nhwc")
    return y


def gconv1x1_wgrad_supported(pixels: int, cin: int, cout: int) -> bool:
    """Shapes and sizes eqa_gconv1x1_wgrad takes -- what `gconv1x1_supported` admits, the size test included."""
    return bool(_lib.load().eqa_gconv1x1_wgrad_supported(pixels, cin, cout))


def gconv1x1_wgrad(x: torch.Tensor, dz: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Filter and bias gradient of z = conv1x1(x) + bias for the output gradient dz (eqa_gconv1x1_wgrad: the contraction over the
    pixels on the fp32 MFMA, split over the chip's waves, partial tiles added in a fixed order in fp64).  x, dz: channels-last
    (B, C, H, W) maps or their (pixels, C) matrices, of the same number of pixels -> (dW (Cout, Cin, 1, 1), dbias (Cout,)).
    No autograd."""
    lib = _lib.load()
    for t, name in ((x, "x"), (dz, "dz")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"gconv1x1_wgrad expects fp32 tensors on the device ({name})")
    if dz.device != x.device or dz.dim() != x.dim():
        raise RuntimeError("gconv1x1_wgrad: x and dz must be on one device and of one layout")

    def rows(t, name):
        if t.dim() == 4:
            if not t.is_contiguous(memory_format=torch.channels_last):
                raise RuntimeError(f"gconv1x1_wgrad: {name} must be a channels-last map, got {tuple(t.shape)} with strides {t.stride()}")
            return t.shape[0] * t.shape[2] * t.shape[3], t.shape[1]
        if t.dim() != 2 or not t.is_contiguous():
            raise RuntimeError(f"gconv1x1_wgrad: {name} must be a contiguous (pixels, channels) matrix, got {tuple(t.shape)}")
        return t.shape[0], t.shape[1]

    (P, Cin), (Pz, Cout) = rows(x, "x"), rows(dz, "dz")
    if Pz != P:
        raise ValueError(f"gconv1x1_wgrad: x has {P} pixels, dz {Pz}")
    if not gconv1x1_wgrad_supported(P, Cin, Cout):
        raise _lib.EqaLibraryError(f"eqa_gconv1x1_wgrad does not take {P} pixels of {Cin} -> {Cout} channels (ask gconv1x1_wgrad_supported first)")
    dW = torch.empty((Cout, Cin, 1, 1), dtype=torch.float32, device=x.device)
    dbias = torch.empty(Cout, dtype=torch.float32, device=x.device)
    nbytes = lib.eqa_gconv1x1_wgrad_workspace_bytes(P, Cin, Cout)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("gconv1x1_wgrad"):
        st = lib.eqa_gconv1x1_wgrad(x.data_ptr(), dz.data_ptr(), dW.data_ptr(), dbias.data_ptr(), work.data_ptr() if nbytes else None,
                                    P, Cin, Cout, _stream())
    _lib.check(st, "eqa_gconv1x1_wgrad")
    return dW, dbias


def conv3x3_supported(n: int, h: int, w: int, cin: int, cout: int, taps: int, stride: int) -> bool:
    """Shapes and sizes eqa_conv3x3_nhwc takes: channel counts on the multiples of 32 from 32 to 512; taps 9 (3 x 3, padding 1) at
    stride 1 or 2, taps 1 (1 x 1, no padding) at stride 2; x, y and res each inside one 32-bit buffer range (the size is part of the
    query: a caller that asks first takes its other route instead of failing in the launch)."""
    return bool(_lib.load().eqa_conv3x3_supported(n, h, w, cin, cout, taps, stride))


def pack_conv3x3_weights(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, k, k) filters, k in {1, 3}, Cin and Cout multiples of 32 -> the MFMA operand-fragment order of eqa_conv3x3_nhwc,
    tap-major, shape (k k, Cin/16, Cout/32, 2, 64, 4):
        Wpk[k dy + dx][s][n][b][32 h + i][t] = w[32 n + i][16 s + 8 b + 4 h + t][dy][dx]
    (`pack_plane_gemm_weights` with the taps as planes).  A pure torch op: it works on any device."""
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3) or w.shape[0] % 32 or w.shape[1] % 32 or not w.numel():
        raise ValueError(f"pack_conv3x3_weights takes (Cout, Cin, k, k) filters, k in (1, 3), channels on multiples of 32, got {tuple(w.shape)}")
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]
    return pack_plane_gemm_weights(w.permute(2, 3, 1, 0).reshape(k * k, Cin, Cout)).reshape(k * k, Cin // 16, Cout // 32, 2, 64, 4)


def conv3x3_nhwc(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, res: Optional[torch.Tensor] = None, relu: bool = False,
                 taps: int = 9, stride: int = 1) -> torch.Tensor:
    """y = [relu](conv(x) + bias [+ res]) in one launch (eqa_conv3x3_nhwc): taps = 9 a 3 x 3 convolution with zero padding 1, taps = 1
    a 1 x 1 one without (stride 2 only).  x: a contiguous (N, H, W, Cin) fp32 map on the device; res and the result (N, OH, OW, Cout)
    with OH = (H + 2 pad - k) // stride + 1; wpk = pack_conv3x3_weights(filters).  No autograd."""
    lib = _lib.load()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError("conv3x3_nhwc expects an fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    if wpk.dim() != 6 or wpk.shape[0] != taps or tuple(wpk.shape[3:]) != (2, 64, 4):
        raise ValueError(f"conv3x3_nhwc: wpk must be pack_conv3x3_weights' ({taps}, Cin/16, Cout/32, 2, 64, 4) operand, got {tuple(wpk.shape)}")
    Cin, Cout = wpk.shape[1] * 16, wpk.shape[2] * 32
    if x.dim() != 4 or x.shape[3] != Cin or not x.is_contiguous():
        raise RuntimeError(f"conv3x3_nhwc: x must be a contiguous (N, H, W, {Cin}) map, got {tuple(x.shape)}")
    N, H, W = x.shape[:3]
    bias = _need(bias, "bias")
    if bias.numel() != Cout:
        raise ValueError(f"conv3x3_nhwc: bias has {Cout} entries")
    if not conv3x3_supported(N, H, W, Cin, Cout, taps, stride):
        raise _lib.EqaLibraryError(f"eqa_conv3x3_nhwc does not take {N} x {H} x {W} maps of {Cin} -> {Cout} channels with taps {taps}, "
                                   f"stride {stride} (ask conv3x3_supported first)")
    k, pad = (3, 1) if taps == 9 else (1, 0)
    out_shape = (N, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, Cout)
    p_res = None
    if res is not None:
        if res.dtype != torch.float32 or res.device != x.device or tuple(res.shape) != out_shape or not res.is_contiguous():
            raise RuntimeError(f"conv3x3_nhwc: res must be a contiguous fp32 {out_shape} map on x's device")
        p_res = res.data_ptr()
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("conv3x3"):
        st = lib.eqa_conv3x3_nhwc(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), p_res, int(relu), y.data_ptr(), N, H, W, Cin, Cout, taps,
                                  stride, _stream())
    _lib.check(st, "eqa_conv3x3_nhwc")
    return y


def convwide_supported(n: int, h: int, w: int, cin: int, cout: int, taps: int, stride: int) -> bool:
    """Shapes and sizes eqa_convwide_nhwc takes: channel counts on the multiples of 32 from 32 to 2048; taps 9 (3 x 3, padding 1) or
    1 (1 x 1, no padding), each at stride 1 or 2; x, y and res each inside one 32-bit buffer range (the size is part of the query)."""
    return bool(_lib.load().eqa_convwide_supported(n, h, w, cin, cout, taps, stride))


def convwide_ksplit(n: int, h: int, w: int, cin: int, cout: int, taps: int, stride: int) -> int:
    """The number of K slices eqa_convwide_nhwc chooses for a shape (ksplit = 0 there): a function of the sizes alone, in
    [1, min(16, taps cin / 32)]; 0 for a shape `convwide_supported` refuses."""
    return int(_lib.load().eqa_convwide_ksplit(n, h, w, cin, cout, taps, stride))


def convwide_nhwc(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, res: Optional[torch.Tensor] = None, relu: bool = False,
                  taps: int = 9, stride: int = 1, ksplit: int = 0) -> torch.Tensor:
    """y = [relu](conv(x) + bias [+ res]) (eqa_convwide_nhwc): `conv3x3_nhwc`'s function and operands on up to 2048 channels, 1 x 1
    at stride 1 included, with the K loop cut into `ksplit` slices (0: the library's choice, `convwide_ksplit`).  ksplit 1 is one
    launch and `conv3x3_nhwc`'s bits; more slices write partial tiles to a workspace allocated here, which a second launch adds in
    a fixed order in fp64.  wpk = pack_conv3x3_weights(filters).  No autograd."""
    lib = _lib.load()
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise RuntimeError("convwide_nhwc expects an fp32 tensor on the device")
    wpk = _need(wpk, "wpk")
    if wpk.dim() != 6 or wpk.shape[0] != taps or tuple(wpk.shape[3:]) != (2, 64, 4):
        raise ValueError(f"convwide_nhwc: wpk must be pack_conv3x3_weights' ({taps}, Cin/16, Cout/32, 2, 64, 4) operand, got {tuple(wpk.shape)}")
    Cin, Cout = wpk.shape[1] * 16, wpk.shape[2] * 32
    if x.dim() != 4 or x.shape[3] != Cin or not x.is_contiguous():
        raise RuntimeError(f"convwide_nhwc: x must be a contiguous (N, H, W, {Cin}) map, got {tuple(x.shape)}")
    N, H, W = x.shape[:3]
    bias = _need(bias, "bias")
    if bias.numel() != Cout:
        raise ValueError(f"convwide_nhwc: bias has {Cout} entries")
    if not convwide_supported(N, H, W, Cin, Cout, taps, stride):
        raise _lib.EqaLibraryError(f"eqa_convwide_nhwc does not take {N} x {H} x {W} maps of {Cin} -> {Cout} channels with taps {taps}, "
                                   f"stride {stride} (ask convwide_supported first)")
    if ksplit == 0:
        ksplit = convwide_ksplit(N, H, W, Cin, Cout, taps, stride)
    if not 1 <= ksplit <= min(16, taps * Cin // 32):
        raise _lib.EqaLibraryError(f"eqa_convwide_nhwc: ksplit {ksplit} is outside [1, {min(16, taps * Cin // 32)}]")
    _, _, OH, OW = _conv3x3_geom(H, W, taps, stride)
    out_shape = (N, OH, OW, Cout)
    p_res = None
    if res is not None:
        if res.dtype != torch.float32 or res.device != x.device or tuple(res.shape) != out_shape or not res.is_contiguous():
            raise RuntimeError(f"convwide_nhwc: res must be a contiguous fp32 {out_shape} map on x's device")
        p_res = res.data_ptr()
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    nbytes = lib.eqa_convwide_workspace_bytes(N, H, W, Cin, Cout, taps, stride, ksplit)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    with torch.cuda.device(x.device), _timed("convwide"):
        st = lib.eqa_convwide_nhwc(x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), p_res, int(relu), y.data_ptr(),
                                   work.data_ptr() if nbytes else None, N, H, W, Cin, Cout, taps, stride, ksplit, _stream())
    _lib.check(st, "eqa_convwide_nhwc")
    return y


def _conv3x3_geom(h: int, w: int, taps: int, stride: int) -> Tuple[int, int, int, int]:
    k, pad = (3, 1) if taps == 9 else (1, 0)
    return k, pad, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def _conv3x3_map(t: torch.Tensor, what: str, name: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
        raise RuntimeError(f"{what}: {name} must be a contiguous (N, H, W, C) fp32 map on the device")
    return t


def conv3x3_wgrad_supported(n: int, h: int, w: int, cin: int, cout: int, taps: int, stride: int) -> bool:
    """Shapes and sizes eqa_conv3x3_wgrad takes -- what `conv3x3_supported` admits, the size test included."""
    return bool(_lib.load().eqa_conv3x3_wgrad_supported(n, h, w, cin, cout, taps, stride))


def conv3x3_wgrad(x: torch.Tensor, dz: torch.Tensor, taps: int = 9, stride: int = 1) -> torch.Tensor:
    """Filter gradient of z = conv3x3_nhwc(x) for the output gradient dz (eqa_conv3x3_wgrad: the contraction over the output pixels
    on the fp32 MFMA, split over the chip's waves, partial tiles added in a fixed order in fp64).  x: a contiguous (N, H, W, Cin)
    map, dz: (N, OH, OW, Cout) -> dW (Cout, Cin, k, k), the layout of `conv.weight`.  No autograd."""
    lib = _lib.load()
    x, dz = _conv3x3_map(x, "conv3x3_wgrad", "x"), _conv3x3_map(dz, "conv3x3_wgrad", "dz")
    N, H, W, Cin = x.shape
    Cout = dz.shape[3]
    if not conv3x3_wgrad_supported(N, H, W, Cin, Cout, taps, stride):
        raise _lib.EqaLibraryError(f"eqa_conv3x3_wgrad does not take {N} x {H} x {W} maps of {Cin} -> {Cout} channels with taps {taps}, "
                                   f"stride {stride} (ask conv3x3_wgrad_supported first)")
    k, _, OH, OW = _conv3x3_geom(H, W, taps, stride)
    if dz.device != x.device or tuple(dz.shape) != (N, OH, OW, Cout):
        raise ValueError(f"conv3x3_wgrad: dz must be a {(N, OH, OW, Cout)} map on x's device, got {tuple(dz.shape)}")
    dW = torch.empty((Cout, Cin, k, k), dtype=torch.float32, device=x.device)
    nbytes = lib.eqa_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout, taps, stride)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("conv3x3_wgrad"):
        st = lib.eqa_conv3x3_wgrad(x.data_ptr(), dz.data_ptr(), work.data_ptr() if nbytes else None, dW.data_ptr(), N, H, W, Cin, Cout,
                                   taps, stride, _stream())
    _lib.check(st, "eqa_conv3x3_wgrad")
    return dW


def conv3x3_dgrad_supported(n: int, h: int, w: int, cin: int, cout: int, taps: int, stride: int) -> bool:
    """Shapes and sizes eqa_conv3x3_dgrad takes (n, h, w: the INPUT map's, as for the forward) -- what `conv3x3_supported` admits."""
    return bool(_lib.load().eqa_conv3x3_dgrad_supported(n, h, w, cin, cout, taps, stride))


def pack_conv3x3_dgrad_weights(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, k, k) filters, k in {1, 3}, Cin and Cout multiples of 32 -> the operand of eqa_conv3x3_dgrad: input and output
    channels exchanged, the taps flipped, in the forward's fragment order, shape (k k, Cout/16, Cin/32, 2, 64, 4):
        Wdpk[k dy + dx][s][n][b][32 h + i][t] = w[16 s + 8 b + 4 h + t][32 n + i][k - 1 - dy][k - 1 - dx]
    (`pack_conv3x3_weights` of the flipped transpose).  A pure torch op: it works on any device."""
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3) or w.shape[0] % 32 or w.shape[1] % 32 or not w.numel():
        raise ValueError(f"pack_conv3x3_dgrad_weights takes (Cout, Cin, k, k) filters, k in (1, 3), channels on multiples of 32, got {tuple(w.shape)}")
    return pack_conv3x3_weights(w.transpose(0, 1).flip(2, 3))


def conv3x3_dgrad(dz: torch.Tensor, wdpk: torch.Tensor, in_hw: Tuple[int, int], res: Optional[torch.Tensor] = None, taps: int = 9,
                  stride: int = 1) -> torch.Tensor:
    """Data gradient of z = conv3x3_nhwc(x) (+ res) in one launch (eqa_conv3x3_dgrad, a mode of the forward kernel): dz a contiguous
    (N, OH, OW, Cout) map, wdpk = pack_conv3x3_dgrad_weights(filters), in_hw = (H, W) of x (OH does not determine H at stride 2);
    res and the result (N, H, W, Cin) -- res is the other branch's gradient at the block input.  No autograd."""
    lib = _lib.load()
    dz = _conv3x3_map(dz, "conv3x3_dgrad", "dz")
    wdpk = _need(wdpk, "wdpk")
    if wdpk.dim() != 6 or wdpk.shape[0] != taps or tuple(wdpk.shape[3:]) != (2, 64, 4) or wdpk.shape[1] * 16 != dz.shape[3]:
        raise ValueError(f"conv3x3_dgrad: wdpk must be pack_conv3x3_dgrad_weights' ({taps}, Cout/16, Cin/32, 2, 64, 4) operand for "
                         f"{dz.shape[3]} output channels, got {tuple(wdpk.shape)}")
    Cout, Cin = wdpk.shape[1] * 16, wdpk.shape[2] * 32
    N, (H, W) = dz.shape[0], in_hw
    if not conv3x3_dgrad_supported(N, H, W, Cin, Cout, taps, stride):
        raise _lib.EqaLibraryError(f"eqa_conv3x3_dgrad does not take {N} x {H} x {W} maps of {Cin} -> {Cout} channels with taps {taps}, "
                                   f"stride {stride} (ask conv3x3_dgrad_supported first)")
    _, _, OH, OW = _conv3x3_geom(H, W, taps, stride)
    if tuple(dz.shape[1:3]) != (OH, OW):
        raise ValueError(f"conv3x3_dgrad: a {H} x {W} input gives a {OH} x {OW} output, dz is {tuple(dz.shape)}")
    p_res = None
    if res is not None:
        if res.dtype != torch.float32 or res.device != dz.device or tuple(res.shape) != (N, H, W, Cin) or not res.is_contiguous():
            raise RuntimeError(f"conv3x3_dgrad: res must be a contiguous fp32 {(N, H, W, Cin)} map on dz's device")
        p_res = res.data_ptr()
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dz.device)
    with torch.cuda.device(dz.device), _timed("conv3x3_dgrad"):
        st = lib.eqa_conv3x3_dgrad(dz.data_ptr(), wdpk.data_ptr(), p_res, dx.data_ptr(), N, H, W, Cin, Cout, taps, stride, _stream())
    _lib.check(st, "eqa_conv3x3_dgrad")
    return dx


def bn_res_act_fwd(z: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, res: Optional[torch.Tensor], relu: bool) -> torch.Tensor:
    """y = [relu](fmaf(scale[c], z, shift[c]) [+ res]) on a channels-last (npix, C) view (eqa_bn_res_act_fwd)."""
    lib = _lib.load()
    z, scale, shift = _need(z, "z"), _need(scale, "scale"), _need(shift, "shift")
    res, p_res = _opt(res, "res", torch.float32)
    if res is not None and res.shape != z.shape:
        raise ValueError(f"bn_res_act_fwd: res is {tuple(res.shape)}, z {tuple(z.shape)}")
    npix, C = z.shape
    y = torch.empty_like(z)
    with torch.cuda.device(z.device), _timed("bn_res_act_fwd"):
        st = lib.eqa_bn_res_act_fwd(z.data_ptr(), scale.data_ptr(), shift.data_ptr(), p_res, int(relu), y.data_ptr(), npix, C, _stream())
    _lib.check(st, "eqa_bn_res_act_fwd")
    return y


def bn_res_act_bwd(gy: torch.Tensor, z: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                   gamma: torch.Tensor, res: Optional[torch.Tensor], relu: bool, need_dres: bool = False):
    """Backward of batch-norm (batch statistics) + residual + ReLU on (npix, C): -> (dz, dgamma, dbeta, dres); dres (= the masked
    gy, written by the pass that writes dz) is None unless `need_dres` (eqa_bn_res_act_bwd_reduce / eqa_bn_act_bwd_finalize /
    eqa_bn_res_act_bwd_apply)."""
    lib = _lib.load()
    gy, z = _need(gy, "gy"), _need(z, "z")
    res, p_res = _opt(res, "res", torch.float32)
    npix, C = z.shape
    if gy.shape != z.shape or (res is not None and res.shape != z.shape):
        raise ValueError(f"bn_res_act_bwd: gy, z and res must be of one shape, got {tuple(gy.shape)}, {tuple(z.shape)}")
    part = torch.empty((max(lib.eqa_bn_act_partial_blocks(npix), 1), C, 2), dtype=torch.float64, device=z.device)
    with torch.cuda.device(z.device), _timed("bn_res_act_bwd_reduce"):
        st = lib.eqa_bn_res_act_bwd_reduce(gy.data_ptr(), z.data_ptr(), scale.data_ptr(), shift.data_ptr(), p_res, int(relu), mean.data_ptr(),
                                           rstd.data_ptr(), part.data_ptr(), npix, C, _stream())
    _lib.check(st, "eqa_bn_res_act_bwd_reduce")
    coef = torch.empty((5, C), dtype=torch.float32, device=z.device)          # dgamma, dbeta, gscale, m1, m2
    with torch.cuda.device(z.device):
        st = lib.eqa_bn_act_bwd_finalize(part.data_ptr(), npix, C, gamma.data_ptr(), rstd.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(),
                                         coef[2].data_ptr(), coef[3].data_ptr(), coef[4].data_ptr(), _stream())
    _lib.check(st, "eqa_bn_act_bwd_finalize")
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if need_dres else None
    with torch.cuda.device(z.device), _timed("bn_res_act_bwd_apply"):
        st = lib.eqa_bn_res_act_bwd_apply(gy.data_ptr(), z.data_ptr(), scale.data_ptr(), shift.data_ptr(), p_res, int(relu), mean.data_ptr(),
                                          rstd.data_ptr(), coef[2].data_ptr(), coef[3].data_ptr(), coef[4].data_ptr(), dz.data_ptr(),
                                          dres.data_ptr() if need_dres else None, npix, C, _stream())
    _lib.check(st, "eqa_bn_res_act_bwd_apply")
    return dz, coef[0], coef[1], dres
