"""High-precision reference of the group action on images and of its derivatives.  TEST INFRASTRUCTURE ONLY.

``action`` restates what ``eqa_group_action_fwd`` computes as a function of ITS OWN arguments
``(src, gidx, theta (E, 6), flags, chan_map, pad, out_hw, top_left)`` -- not of a group, an angle or a module -- as one chain of
differentiable torch-CPU ops:

    channel map -> flip the source (FLIP_SRC) -> replicate-pad -> F.affine_grid(align_corners=True)
    -> F.grid_sample(bilinear, zeros, align_corners=True) -> flip the frame (FLIP_DST) -> crop [top:top+OH, left:left+OW]

(The frame is flipped BEFORE the crop, as the kernels' ``frame_x`` does; for a crop that is centred in the frame -- every use of
FLIP_DST in the package and in the tests -- that equals cropping first.)  Output channel ``c`` of a mapped action reads source
channel ``(c // G) * G + chan_map[e, c % G]``.

``theta`` is taken as the kernel gets it: the values of the fp32 table, cast to ``dtype``, never recomputed from angles.  Run in
``float64`` the chain is the reference; autograd through it gives dL/dsrc and dL/dtheta (all six components per OUTPUT image).  The
same function run in ``float32`` is the "fp32 CPU chain": an independent fp32 evaluation of the same expression, whose distance
from the fp64 result is what an fp32 kernel may be expected to reach (tests/action_backward_cases.py sizes its budgets with it).

The gradient with respect to the ROTATION ANGLE (degrees) is dL/dtheta contracted with d rotation_theta / d angle, the Jacobian
taken by autograd through ``rotation_theta`` below, an fp64 restatement of ``equiadapt_amd.images.geometry.rotation_theta``.
"""
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

FLIP_SRC = 1
FLIP_DST = 2


class ActionResult(NamedTuple):
    out: torch.Tensor                   # (n_out, C, OH, OW)
    ix: torch.Tensor                    # (n_out, OH, OW) sample point of every output pixel, frame pixels
    iy: torch.Tensor
    frame: Optional[torch.Tensor]       # the padded (mapped, flipped) frame the samples were taken from, when asked for


def rotation_theta(angles_deg: torch.Tensor, frame_hw: Tuple[int, int], dtype=torch.float64,
                   center: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    """(E,) angles in degrees -> (E, 6): the matrix ``rotate(img, angle)`` hands to ``F.affine_grid`` on an (Hp, Wp) frame.

    The op chain of ``geometry.rotation_theta`` (rotation matrix about ``center`` -> normalise -> inverse), differentiable in
    the angles.  ``center`` defaults to kornia's ((Wp - 1) / 2, (Hp - 1) / 2); another value is for planting errors in tests."""
    Hp, Wp = frame_hw
    a = torch.deg2rad(angles_deg.to(dtype).reshape(-1))
    cos_a, sin_a = torch.cos(a), torch.sin(a)
    cx, cy = ((Wp - 1) / 2.0, (Hp - 1) / 2.0) if center is None else center
    zero, one = torch.zeros_like(a), torch.ones_like(a)
    M = torch.stack([torch.stack([cos_a, sin_a, (1.0 - cos_a) * cx - sin_a * cy], dim=-1),
                     torch.stack([-sin_a, cos_a, sin_a * cx + (1.0 - cos_a) * cy], dim=-1),
                     torch.stack([zero, zero, one], dim=-1)], dim=1)                      # (E, 3, 3) pixel space, dst <- src
    norm = torch.tensor([[2.0 / (Wp - 1.0), 0.0, -1.0], [0.0, 2.0 / (Hp - 1.0), -1.0], [0.0, 0.0, 1.0]], dtype=dtype)
    dst_norm_from_src_norm = norm @ (M @ torch.linalg.inv(norm))
    return torch.linalg.inv(dst_norm_from_src_norm)[:, :2, :].reshape(-1, 6)


def rotation_theta_jacobian(angles_deg: torch.Tensor, frame_hw: Tuple[int, int],
                            center: Optional[Tuple[float, float]] = None) -> torch.Tensor:
    """d rotation_theta / d angle, per degree, in fp64: (E, 6).  Row e depends on angle e alone."""
    ang = angles_deg.detach().double().reshape(-1)
    J = torch.autograd.functional.jacobian(lambda t: rotation_theta(t, frame_hw, torch.float64, center), ang)   # (E, 6, E)
    idx = torch.arange(ang.shape[0])
    return J[idx, :, idx]


def element_of_output(gidx: Optional[torch.Tensor], E: int, B: int):
    """(element index, source image index) of every output image: ``gidx`` given -> (gidx[n], n); orbit mode -> n = e * B + b."""
    if gidx is not None:
        return gidx.long().clamp(0, E - 1), torch.arange(gidx.shape[0])
    n = torch.arange(E * B)
    return n // B, n % B


def action(src: torch.Tensor, gidx: Optional[torch.Tensor], theta: torch.Tensor, flags: Optional[torch.Tensor],
           chan_map: Optional[torch.Tensor], pad: int, out_hw: Tuple[int, int], top_left: Tuple[int, int],
           dtype=torch.float64, theta_rows: Optional[torch.Tensor] = None, keep_frame: bool = False) -> ActionResult:
    """The action in ``dtype``.  ``theta_rows``: the (n_out, 6) matrices already gathered per output image (a leaf whose
    ``.grad`` is then dL/dtheta per output image); default ``theta[element of n]``.  ``keep_frame``: retain the padded frame
    (and, under autograd, its gradient: the input gradient before the adjoint of the padding)."""
    B, C, H, W = src.shape
    E = theta.shape[0]
    e, b = element_of_output(gidx, E, B)
    n_out = e.shape[0]
    x = src.to(dtype)[b]
    if chan_map is not None:
        G = chan_map.shape[1]
        c = torch.arange(C)
        cs = (c // G)[None, :] * G + chan_map.long()[e][:, c % G]                       # (n_out, C)
        x = x[torch.arange(n_out)[:, None], cs]
    fl = flags.long()[e] if flags is not None else torch.zeros(n_out, dtype=torch.long)
    flip_src, flip_dst = (fl & FLIP_SRC) != 0, (fl & FLIP_DST) != 0
    x = torch.where(flip_src[:, None, None, None], x.flip(-1), x)
    frame = F.pad(x, (pad, pad, pad, pad), mode="replicate") if pad > 0 else x
    if keep_frame and frame.requires_grad:
        frame.retain_grad()
    rows = theta.to(dtype)[e] if theta_rows is None else theta_rows
    grid = F.affine_grid(rows.view(-1, 2, 3), list(frame.shape), align_corners=True)
    y = F.grid_sample(frame, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    Hp, Wp = frame.shape[-2:]
    ix = (grid[..., 0].detach() + 1.0) * 0.5 * (Wp - 1)
    iy = (grid[..., 1].detach() + 1.0) * 0.5 * (Hp - 1)
    y = torch.where(flip_dst[:, None, None, None], y.flip(-1), y)
    ix = torch.where(flip_dst[:, None, None], ix.flip(-1), ix)
    iy = torch.where(flip_dst[:, None, None], iy.flip(-1), iy)
    (top, left), (OH, OW) = top_left, out_hw
    crop = (slice(None), slice(top, top + OH), slice(left, left + OW))
    return ActionResult(y[:, :, top:top + OH, left:left + OW], ix[crop], iy[crop], frame if keep_frame else None)


class ActionGrads(NamedTuple):
    out: torch.Tensor                   # (n_out, C, OH, OW), detached
    d_src: torch.Tensor                 # (B, C, H, W) fp64
    d_theta: torch.Tensor               # (n_out, 6) fp64
    d_frame: Optional[torch.Tensor]     # (n_out, C, Hp, Wp) fp64 when asked for


def action_grads(src, grad_out, gidx, theta, flags, chan_map, pad, top_left, dtype=torch.float64,
                 keep_frame: bool = False) -> ActionGrads:
    """Backward of ``action`` by autograd, evaluated in ``dtype`` and returned in fp64: dL/dsrc and dL/dtheta per output image
    for L = <action(src), grad_out>."""
    x = src.detach().to(dtype).clone().requires_grad_(True)
    e, _ = element_of_output(gidx, theta.shape[0], src.shape[0])
    rows = theta.detach().to(dtype)[e].clone().requires_grad_(True)
    res = action(x, gidx, theta, flags, chan_map, pad, tuple(grad_out.shape[-2:]), top_left, dtype, theta_rows=rows,
                 keep_frame=keep_frame)
    (res.out * grad_out.to(dtype)).sum().backward()
    d_frame = res.frame.grad.double() if keep_frame and res.frame is not None and res.frame.grad is not None else None
    return ActionGrads(res.out.detach().double(), x.grad.double(), rows.grad.double(), d_frame)


def off_kink_mask(ix: torch.Tensor, iy: torch.Tensor, margin: float = 2.0 ** -9) -> torch.Tensor:
    """True where the sample point keeps ``margin`` pixels from every source grid line.  The bilinear interpolant has a kink on
    the grid lines: d value / d coordinate jumps there, and which side an fp32 sample point falls on is decided by its last
    bits.  Zeroing the output gradient elsewhere removes those terms from the reference and from the kernel alike (the
    gradients are linear in the output gradient)."""
    dx = (ix - torch.round(ix)).abs()
    dy = (iy - torch.round(iy)).abs()
    return (dx >= margin) & (dy >= margin)
