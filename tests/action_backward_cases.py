"""Cases, references, measures and budgets shared by tests/test_gpu_action_backward_fp64.py (the kernels) and
tests/test_action_fp64_reference.py (the reference's conventions, and planted errors that the measures must catch).

Everything here runs on the CPU and knows nothing about the kernels.  A "measure" takes a candidate result and the fp64
reference and returns one relative error; a "budget" is M = 4 times the error of the fp32 CPU chain (oracle/action_fp64.py run in
float32: torch's own fp32 evaluation of the same expression) under the same measure, pooled -- the worst -- over all cases of
this file, so that one lucky case cannot yield a near-zero budget.  Both sides of the comparison are then fp32 evaluations of
the same expression with sums of comparable length; the kernels add in tile and wave order, torch in its own: 4 leaves room for
the order of the additions and for nothing else.

Inputs for which the reference is unambiguous: the angle and theta gradients use smooth images and an output gradient that is
zero wherever the fp64 sample point lies within 2**-9 px of a source grid line (oracle.action_fp64.off_kink_mask: 30 x the fp32
coordinate error at coordinate 448); no angle is a multiple of 90 degrees and the frames of those cases have even sides, so
the rotation centre sits on a half pixel and 45 degrees puts nothing on the grid.  The input gradient has no kink: white noise
and a full output gradient.
"""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import torch

from equiadapt_amd.images import geometry
from oracle import action_fp64 as ref

M_BUDGET = 4.0
KINK_MARGIN = 2.0 ** -9
MAX_ZEROED = 0.03
ANGLES = (17.0, 45.0, 101.3, -63.0, 135.0, 200.7, 225.0, 315.0, 3.0, 88.0, 271.5)


class Case(NamedTuple):
    name: str
    B: int
    C: int
    H: int
    W: int
    pad: int
    out_hw: Tuple[int, int]
    top_left: Tuple[int, int]
    tables: Optional[str] = None     # which geometry table supplies flags / chan_map (and, for "d4-invert", run A's thetas)
    theta_case: bool = False         # also run for the theta gradient (per-sample rows, no flags, no channel map)


CASES = (
    Case("padded-w90", 11, 3, 70, 90, 45, (70, 90), (45, 45), theta_case=True),     # 3 x 3 ragged tiles, 8 + 3 images, scalar stores
    Case("padded-w96", 8, 2, 64, 96, 48, (64, 96), (48, 48), theta_case=True),      # exact tiles, two channels per stage
    Case("off-centre-crop", 3, 5, 70, 90, 45, (40, 51), (38, 52), theta_case=True),  # one channel per stage, ragged group only
    Case("unpadded-c8-mapped", 11, 8, 96, 64, 0, (96, 64), (0, 0), tables="c8-invert"),
    Case("unpadded-d4", 8, 16, 96, 64, 0, (96, 64), (0, 0), tables="d4-invert"),
    Case("canonicalize-d4", 8, 3, 64, 64, 32, (64, 64), (32, 32), tables="d4-canonicalize"),
    Case("224-unpadded", 3, 3, 224, 224, 0, (224, 224), (0, 0), theta_case=True),   # 7 x 7 tiles
    Case("224-padded", 3, 3, 224, 224, 112, (224, 224), (112, 112), theta_case=True),  # the training shape's frame
)
CASE_BY_NAME = {c.name: c for c in CASES}
THETA_CASES = tuple(c for c in CASES if c.theta_case)


def smooth(B, C, H, W, seed):
    """Low-frequency images with per-(sample, channel) phases and frequencies (the `_smooth` of tests/test_gpu_backward.py)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.rand(B, C, 1, 1, generator=g) * 6.28
    fx = 0.05 + 0.1 * torch.rand(B, C, 1, 1, generator=g)
    fy = 0.05 + 0.1 * torch.rand(B, C, 1, 1, generator=g)
    return (torch.sin(fx * xx + ph) * torch.cos(fy * yy - ph) + 0.02 * xx - 0.01 * yy).contiguous()


def frame_hw(case: Case) -> Tuple[int, int]:
    return case.H + 2 * case.pad, case.W + 2 * case.pad


def angles_of(case: Case) -> torch.Tensor:
    return torch.tensor(ANGLES[:case.B])


def affine_rows(case: Case) -> torch.Tensor:
    """General affine rows: the rotation rows with the linear part scaled by 0.8 + 0.05 b, a translation of
    (0.02 cos b, 0.03 sin b) in normalised units, and row 0 times 1.1 -- all six components move independently."""
    th = geometry.rotation_theta(angles_of(case), frame_hw(case)).view(-1, 2, 3).clone()
    b = torch.arange(case.B, dtype=torch.float32)
    th[:, :, :2] *= (0.8 + 0.05 * b).view(-1, 1, 1)
    th[:, 0, 2] += 0.02 * torch.cos(b)
    th[:, 1, 2] += 0.03 * torch.sin(b)
    th[:, 0, :] *= 1.1
    return th.reshape(-1, 6).contiguous()


class Setup(NamedTuple):
    """The arguments of one call, as the kernel gets them (CPU tensors)."""
    case: Case
    gidx: torch.Tensor                   # int32 (B,)
    theta: torch.Tensor                  # fp32 (E, 6)
    flags: Optional[torch.Tensor]        # int32 (E,)
    chan_map: Optional[torch.Tensor]     # int32 (E, G)


def _tables(case: Case):
    """(table thetas or None, flags, chan_map) for a case; rows are indexed by gidx = arange(B)."""
    fr = frame_hw(case)
    if case.tables is None:
        return None, None, None
    if case.tables == "c8-invert":       # the C8 channel maps, one row per output image (B = 11 > 8 elements: rows repeat)
        _, _, cm = geometry.invert_tables(8, False, fr)
        return None, None, cm[torch.arange(case.B) % 8].contiguous()
    if case.tables == "d4-invert":       # FLIP_DST for the first four elements, regular D4 channel maps (G = 8)
        th, fl, cm = geometry.invert_tables(4, True, fr)
        return th, fl, cm
    if case.tables == "d4-canonicalize":  # FLIP_SRC for the last four elements
        th, fl = geometry.canonicalize_tables(4, True, fr)
        return th, fl, None
    raise ValueError(case.tables)


def setup(case: Case, rows: str = "rotation") -> Setup:
    """rows: "rotation" = geometry.rotation_theta of this file's angles; "table" = the group table's own elements (right
    angles; the input gradient of the un-padded D4 case); "affine" = affine_rows."""
    th_table, flags, cmap = _tables(case)
    if rows == "rotation":
        theta = geometry.rotation_theta(angles_of(case), frame_hw(case))
    elif rows == "table":
        theta = th_table.clone()
    elif rows == "affine":
        assert flags is None and cmap is None
        theta = affine_rows(case)
    else:
        raise ValueError(rows)
    assert theta.shape[0] == case.B
    return Setup(case, torch.arange(case.B, dtype=torch.int32), theta.contiguous(), flags, cmap)


def input_gradient_rows(case: Case) -> str:
    return "table" if case.tables == "d4-invert" else "rotation"


# ---- inputs ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def noise_inputs(name: str):
    """White-noise source and full output gradient: the input gradient's inputs."""
    c = CASE_BY_NAME[name]
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    return torch.randn(c.B, c.C, c.H, c.W, generator=g), torch.randn(c.B, c.C, *c.out_hw, generator=g)


@functools.lru_cache(maxsize=None)
def smooth_inputs(name: str, rows: str):
    """Smooth source and an output gradient zeroed near the kinks of the fp64 sample points: the inputs of the angle and theta
    gradients.  Returns (src, grad_out, share of zeroed output pixels per image)."""
    c = CASE_BY_NAME[name]
    s = setup(c, rows)
    src = smooth(c.B, c.C, c.H, c.W, 2000 + CASES.index(c))
    g = torch.Generator().manual_seed(3000 + CASES.index(c))
    gy = torch.randn(c.B, c.C, *c.out_hw, generator=g)
    with torch.no_grad():
        res = ref.action(src, s.gidx, s.theta, s.flags, s.chan_map, c.pad, c.out_hw, c.top_left, torch.float64)
    keep = ref.off_kink_mask(res.ix, res.iy, KINK_MARGIN)
    zeroed = 1.0 - keep.double().mean(dim=(1, 2))
    return src, (gy * keep[:, None].float()).contiguous(), zeroed


def check_inputs_are_unambiguous(name: str, rows: str) -> float:
    """The conditions on the inputs, asserted on the reference alone.  Returns the largest share of zeroed pixels."""
    c = CASE_BY_NAME[name]
    Hp, Wp = frame_hw(c)
    assert Hp % 2 == 0 and Wp % 2 == 0, (name, Hp, Wp)
    assert all(math.fmod(a, 90.0) != 0.0 for a in ANGLES[:c.B]), name
    zeroed = smooth_inputs(name, rows)[2]
    assert zeroed.max().item() <= MAX_ZEROED, (name, rows, zeroed.tolist())
    return zeroed.max().item()


# ---- references -----------------------------------------------------------------------------------------------------------


class Reference(NamedTuple):
    f64: ref.ActionGrads
    f32: ref.ActionGrads


def _both(src, gy, s: Setup, keep_frame=False) -> Reference:
    c = s.case
    args = (src, gy, s.gidx, s.theta, s.flags, s.chan_map, c.pad, c.top_left)
    return Reference(ref.action_grads(*args, dtype=torch.float64, keep_frame=keep_frame),
                     ref.action_grads(*args, dtype=torch.float32, keep_frame=keep_frame))


def input_gradient_row_sets(case: Case) -> Tuple[str, ...]:
    """Row sets the input gradient runs on.  A pure rotation of a centred crop of the source's own size never reaches the
    corner blocks of the padding (the source's corners are the farthest points from the centre that it can touch); the affine
    rows' scales above 1 do, so the padded theta cases hold the corners of the padding's adjoint through them."""
    return (input_gradient_rows(case),) + (("affine",) if case.theta_case else ())


@functools.lru_cache(maxsize=None)
def input_gradient_reference(name: str, rows: str, keep_frame: bool = False) -> Reference:
    src, gy = noise_inputs(name)
    return _both(src, gy, setup(CASE_BY_NAME[name], rows), keep_frame)


@functools.lru_cache(maxsize=None)
def transform_gradient_reference(name: str, rows: str) -> Reference:
    src, gy, _ = smooth_inputs(name, rows)
    return _both(src, gy, setup(CASE_BY_NAME[name], rows))


@functools.lru_cache(maxsize=None)
def angle_jacobian(name: str) -> torch.Tensor:
    c = CASE_BY_NAME[name]
    return ref.rotation_theta_jacobian(angles_of(c), frame_hw(c))


def angle_gradient(d_theta: torch.Tensor, jac: torch.Tensor) -> torch.Tensor:
    """dL/d angle per degree = <dL/dtheta, d rotation_theta / d angle>, per output image."""
    return (d_theta.double() * jac).sum(dim=1)


# ---- measures -------------------------------------------------------------------------------------------------------------

REGIONS = ("interior", "borders", "corners")


def _region_masks(H: int, W: int):
    edge = torch.zeros(H, W, dtype=torch.bool)
    edge[0, :] = edge[-1, :] = True
    edge[:, 0] = edge[:, -1] = True
    corner = torch.zeros(H, W, dtype=torch.bool)
    corner[0, 0] = corner[0, -1] = corner[-1, 0] = corner[-1, -1] = True
    return {"interior": ~edge, "borders": edge & ~corner, "corners": corner}


def measure_input_gradient(got: torch.Tensor, want: torch.Tensor) -> dict:
    """max |got - want| over the interior pixels, the four border lines and the four corners, each relative to that region's own
    max |want| (the adjoint of the padding piles pad^2 terms on a corner: one norm over everything would hide the interior)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape
    out = {}
    for k, m in _region_masks(*want.shape[-2:]).items():
        diff, scale = (got - want)[..., m].abs().max().item(), want[..., m].abs().max().item()
        # (a region nothing reaches -- the corners under a pure rotation -- is exactly zero in the reference: so must it be in `got`)
        out[k] = diff / scale if scale > 0.0 else (0.0 if diff == 0.0 else math.inf)
    return out


def measure_per_image(got: torch.Tensor, want: torch.Tensor) -> float:
    """Angle gradient: max over images of |got - want|, relative to max |want|."""
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    assert got.shape == want.shape
    return ((got - want).abs().max() / want.abs().max()).item()


def measure_theta_gradient(got: torch.Tensor, want: torch.Tensor) -> float:
    """Theta gradient: measure_per_image for each of the six components (their scales differ by half_w against half_h), the
    worst of them."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape and want.shape[1] == 6
    return ((got - want).abs().amax(dim=0) / want.abs().amax(dim=0)).max().item()


def measure_forward(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape
    return ((got - want).abs().max() / want.abs().max()).item()


# ---- the fp32 CPU chain's own errors, per case, and the pooled budgets ----------------------------------------------------


@functools.lru_cache(maxsize=None)
def cpu_chain_errors() -> dict:
    """{(quantity, case name[, rows]): error of the fp32 CPU chain against fp64 under the quantity's measure}."""
    err = {}
    for c in CASES:
        for rows in input_gradient_row_sets(c):
            r = input_gradient_reference(c.name, rows)
            for region, v in measure_input_gradient(r.f32.d_src, r.f64.d_src).items():
                err[("input:" + region, c.name, rows)] = v
        t = transform_gradient_reference(c.name, "rotation")
        jac = angle_jacobian(c.name)
        err[("angle", c.name)] = measure_per_image(angle_gradient(t.f32.d_theta, jac), angle_gradient(t.f64.d_theta, jac))
    for c in THETA_CASES:
        for rows in ("rotation", "affine"):
            t = transform_gradient_reference(c.name, rows)
            err[("theta", c.name, rows)] = measure_theta_gradient(t.f32.d_theta, t.f64.d_theta)
        t = transform_gradient_reference(c.name, "affine")
        err[("forward", c.name)] = measure_forward(t.f32.out, t.f64.out)
    return err


@functools.lru_cache(maxsize=None)
def budgets() -> dict:
    """{quantity: M x the worst fp32 CPU chain error of that quantity over this file's cases}."""
    pooled = {}
    for key, v in cpu_chain_errors().items():
        pooled[key[0]] = max(pooled.get(key[0], 0.0), v)
    return {q: M_BUDGET * v for q, v in pooled.items()}
