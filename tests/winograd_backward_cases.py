"""Cases, references, measures and budgets shared by tests/test_gpu_winograd_backward_fp64.py (the kernels and the Python route
of images/canonicalization_networks/winograd.py) and tests/test_winograd_fp64_reference.py (the references against autograd,
and planted errors that the measures must catch).

Everything here runs on the CPU and calls nothing of libeqa_hip.so; of the package it uses the rational Cook-Toom matrices
(``winograd.cook_toom``) and the signs the kernels give B^T's rows (``winograd.kernel_bt_signs``), which tests/test_abi_and_host.py
checks in exact arithmetic.

References, both fp64, on inputs rounded to fp32 first (both sides see the same numbers):
  (a) ``F.conv2d`` through autograd: d_bank and d_x of  y = conv2d(x, bank)  under the output gradient dy;
  (b) the two transforms on their own, in the (tiles, P, C) layout the kernels write, tile = (img * TY + ty) * TX + tx,
      P index = i * N + j:   dM = A dY A^T per m x m tile,   V = B^T d B per (m+4) x (m+4) window of the zero-padded map.

The fp32 CPU chain (``chain(..., torch.float32)``) is the same algorithm as the product's -- input transform, one product per
plane, output transform; the input gradient as the convolution of the zero-padded dy with the flipped, transposed bank; the
filter gradient as dU[a] = V[:, a]^T dM[:, a] folded back with G -- in torch's fp32 CPU ops, with U = G g G^T and G^T dU G in
fp64 as the product does.  A budget is M = 4 times that chain's error against reference (a), relative to the largest reference
entry, pooled (the worst) over all cases and both tile sizes; the 4 leaves room for another order of the additions in the GEMMs
and in the kernels' factored wino_a / wino_bt, and for nothing else.  Nothing is taken from the kernels.

The two transforms alone are held to an a-priori bound instead: with u = 2**-24, any evaluation of  T d T^T  whose sums have
at most eight terms per axis (N <= 8) and whose coefficients keep their magnitudes -- the kernels' factored forms do: they group
terms, they do not cancel coefficients -- errs by at most  gamma * (|T| |d| |T|^T)  elementwise: a sum of at most eight
products errs by (1 + u)^9 - 1 of the sum of their magnitudes in any order, the second axis does so again on the first
one's magnitudes, together less than 19 u.  The bound
used is 64 u, three times that (torch's own fp32 einsum measures 0.03 - 0.05 of it).  A wrong coefficient, sign, tile index or
dropped tap is off by O(1) of |T| |d| |T|^T, some 1e5 times the bound.
"""
import functools
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from equiadapt_amd.images.canonicalization_networks import winograd

M_BUDGET = 4.0
TRANSFORM_GAMMA = 64.0 * 2.0 ** -24
BORDER = 4                    # the outer pixels of d_x that see the zero padding of dy (kernel size - 1)
FORWARD_BOUND = 2e-5          # tests/test_gpu_parity.py::test_winograd_conv_matches_direct


class Case(NamedTuple):
    name: str
    B: int
    Cin: int
    Cout: int
    H: int
    W: int


# What each case reaches in csrc/winograd.hip and winograd.py is listed in tests/test_gpu_winograd_backward_fp64.py and asserted
# in tests/test_winograd_fp64_reference.py (`launch_plan`, `chunk_sizes`).  All maps admit m = 4: every case runs both tile sizes.
CASES = (
    Case("off-32", 3, 32, 48, 12, 16),           # library-GEMM route both ways, non-square, no strips
    Case("strips", 3, 32, 32, 32, 40),           # m = 4 plain: TX = 9, strips (5, 4)
    Case("strips-padded", 3, 32, 32, 36, 44),    # dy 32 x 40: padded m = 4 TX = 11, strips (6, 5), 54 blocks; m = 2 TX = 22, 5,5,5,5,2, 270
    Case("wide", 2, 288, 320, 12, 12),           # second, partly filled channel block in every kernel
    Case("chunks", 9, 32, 64, 12, 12),           # with CHUNK_IMAGES = 2: five chunks of 2 (m = 2), 8 + 1 (m = 4)
)
CASE_BY_NAME = {c.name: c for c in CASES}
TILES = (2, 4)


def tiles_of(case: Case) -> Tuple[int, ...]:
    return tuple(m for m in TILES if (case.H - 4) % m == 0 and (case.W - 4) % m == 0 and case.H >= m + 4 and case.W >= m + 4)


def launch_plan(nimg: int, Hl: int, Wl: int, C: int, m: int) -> dict:
    """What launch_wino_input (csrc/winograd.hip) makes of a logical (padded) Hl x Wl map: tile counts, channel blocks, the
    lengths of the strips of one tile row and the number of work items (blocks per channel block).  Restated here so that the
    tests can say -- and check -- which paths of the kernel a case reaches."""
    TY, TX = (Hl - 4) // m, (Wl - 4) // m
    cb = (C + 255) // 256
    rows = nimg * TY
    nstrip = (4096 + rows * cb - 1) // (rows * cb)
    nstrip = max(1, min(nstrip, max(1, TX // 4)))
    strip_len = (TX + nstrip - 1) // nstrip
    nstrip = (TX + strip_len - 1) // strip_len
    return {"TY": TY, "TX": TX, "channel_blocks": cb, "last_block_lanes": C - 256 * (cb - 1),
            "strips": tuple(min(strip_len, TX - s * strip_len) for s in range(nstrip)), "nwork": rows * nstrip}


def chunk_sizes(B: int, m: int, chunk_images: int) -> Tuple[int, ...]:
    """The image counts of the chunks winograd.conv5x5 / filter_grad walk (chunk_images: winograd.CHUNK_IMAGES)."""
    chunk = min(chunk_images * (m * m // 4), B)
    return tuple(min(chunk, B - b0) for b0 in range(0, B, chunk))


# ---- the matrices ---------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def matrices(m: int):
    """(A^T (m, N), G (N, 5), B^T (N, N)) in fp64 with the kernels' row signs; A^T and B^T are exact in fp32 as well."""
    at, g, bt = winograd.cook_toom(m)
    sg = winograd.kernel_bt_signs(m)
    f = lambda rows, signs: torch.tensor([[float(s * v) for v in row] for s, row in zip(signs, rows)], dtype=torch.float64)  # noqa: E731
    AT, G, BT = f(at, [1] * m), f(g, sg), f(bt, sg)
    assert torch.equal(AT.float().double(), AT) and torch.equal(BT.float().double(), BT)
    return AT, G, BT


# ---- the transforms, in any dtype (reference (b) in fp64, the chain's steps in fp32) ------------------------------------------


def _windows(d: torch.Tensor, m: int, pad: int) -> torch.Tensor:
    """(B, C, H, W) -> (B, TY, TX, C, N, N): the (m+4)^2 windows, stride m, of d zero-padded by `pad`."""
    n = m + 4
    if pad:
        d = F.pad(d, (pad, pad, pad, pad))
    assert (d.shape[-2] - 4) % m == 0 and (d.shape[-1] - 4) % m == 0
    return d.unfold(2, n, m).unfold(3, n, m).permute(0, 2, 3, 1, 4, 5)


def input_transform(d: torch.Tensor, m: int, pad: int = 0, absolute: bool = False) -> torch.Tensor:
    """V (tiles, P, C) = B^T d B per window; ``absolute``: |B^T| |d| |B| (the a-priori bound's right-hand side)."""
    BT = matrices(m)[2].to(d.dtype)
    w = _windows(d, m, pad)
    if absolute:
        BT, w = BT.abs(), w.abs()
    v = torch.einsum("ik,byxckl,jl->byxijc", BT, w, BT)
    return v.reshape(-1, (m + 4) ** 2, d.shape[1]).contiguous()


def output_adjoint(dy: torch.Tensor, m: int, absolute: bool = False) -> torch.Tensor:
    """dM (tiles, P, C) = A dY A^T per m x m tile."""
    A = matrices(m)[0].t().to(dy.dtype)
    B, C, OH, OW = dy.shape
    assert OH % m == 0 and OW % m == 0
    t = dy.reshape(B, C, OH // m, m, OW // m, m)
    if absolute:
        A, t = A.abs(), t.abs()
    dm = torch.einsum("ir,bcyrxq,jq->byxijc", A, t, A)
    return dm.reshape(-1, (m + 4) ** 2, C).contiguous()


def output_transform(M: torch.Tensor, m: int, B: int, TY: int, TX: int) -> torch.Tensor:
    """y (B, C, m TY, m TX) = A^T M A per tile."""
    AT = matrices(m)[0].to(M.dtype)
    n = m + 4
    y = torch.einsum("ri,byxijc,qj->bcyrxq", AT, M.reshape(B, TY, TX, n, n, M.shape[-1]), AT)
    return y.reshape(B, M.shape[-1], TY * m, TX * m)


def transform_filters(bank: torch.Tensor, m: int, dtype) -> torch.Tensor:
    """U (P, Cin, Cout) = G g G^T in fp64, then rounded to the chain's dtype (the product: fp32)."""
    G = matrices(m)[1]
    u = torch.einsum("ak,oikl,bl->abio", G, bank.double(), G)
    return u.reshape((m + 4) ** 2, bank.shape[1], bank.shape[0]).to(dtype)


def fold_back(dU: torch.Tensor, m: int, dtype) -> torch.Tensor:
    """d_bank (Cout, Cin, 5, 5) = G^T dU G in fp64, then rounded to the chain's dtype."""
    G = matrices(m)[1]
    n = m + 4
    return torch.einsum("ak,bl,abio->oikl", G, G, dU.double().reshape(n, n, dU.shape[1], dU.shape[2])).to(dtype)


def _conv(x: torch.Tensor, bank: torch.Tensor, m: int, pad: int, dtype) -> torch.Tensor:
    B, _, H, W = x.shape
    TY, TX = (H + 2 * pad - 4) // m, (W + 2 * pad - 4) // m
    V = input_transform(x.to(dtype), m, pad)
    M = torch.bmm(V.permute(1, 0, 2), transform_filters(bank, m, dtype)).permute(1, 0, 2)
    return output_transform(M, m, B, TY, TX)


class Grads(NamedTuple):
    y: torch.Tensor
    d_bank: torch.Tensor
    d_x: torch.Tensor


def chain(x: torch.Tensor, bank: torch.Tensor, dy: torch.Tensor, m: int, dtype) -> Grads:
    """The Winograd forward and both gradients, evaluated in `dtype` with torch's CPU ops."""
    y = _conv(x, bank, m, 0, dtype)
    V, dM = input_transform(x.to(dtype), m), output_adjoint(dy.to(dtype), m)
    dU = torch.bmm(V.permute(1, 2, 0), dM.permute(1, 0, 2))
    bank_t = bank.flip(-1, -2).transpose(0, 1).contiguous()
    return Grads(y, fold_back(dU, m, dtype), _conv(dy, bank_t, m, 4, dtype))


# ---- inputs and references ------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """(x, bank, dy) in fp32 from a fixed seed; bank = randn / (5 sqrt(Cin)) keeps y at unit scale."""
    c = CASE_BY_NAME[name]
    g = torch.Generator().manual_seed(4000 + CASES.index(c))
    x = torch.randn(c.B, c.Cin, c.H, c.W, generator=g)
    bank = torch.randn(c.Cout, c.Cin, 5, 5, generator=g) / (5.0 * c.Cin ** 0.5)
    dy = torch.randn(c.B, c.Cout, c.H - 4, c.W - 4, generator=g)
    return x, bank, dy


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Grads:
    """Reference (a): fp64 F.conv2d and its autograd gradients."""
    x, bank, dy = (t.double() for t in inputs(name))
    x.requires_grad_(True)
    bank.requires_grad_(True)
    y = F.conv2d(x, bank)
    d_x, d_bank = torch.autograd.grad(y, (x, bank), dy)
    return Grads(y.detach(), d_bank, d_x)


@functools.lru_cache(maxsize=None)
def chain_results(name: str, m: int, fp64: bool = False) -> Grads:
    x, bank, dy = inputs(name)
    with torch.no_grad():
        return chain(x, bank, dy, m, torch.float64 if fp64 else torch.float32)


class TransformReference(NamedTuple):
    want: torch.Tensor      # fp64
    bound: torch.Tensor     # TRANSFORM_GAMMA * |T| |d| |T|^T, fp64


@functools.lru_cache(maxsize=None)
def adjoint_reference(name: str, m: int) -> TransformReference:
    """Reference (b) for eqa_winograd_f{m}k5_output_adjoint on the case's dy."""
    dy = inputs(name)[2].double()
    return TransformReference(output_adjoint(dy, m), TRANSFORM_GAMMA * output_adjoint(dy, m, absolute=True))


@functools.lru_cache(maxsize=None)
def padded_input_reference(name: str, m: int) -> TransformReference:
    """Reference (b) for eqa_winograd_f{m}k5_input_padded (pad = 4) on the case's dy."""
    dy = inputs(name)[2].double()
    return TransformReference(input_transform(dy, m, 4), TRANSFORM_GAMMA * input_transform(dy, m, 4, absolute=True))


@functools.lru_cache(maxsize=None)
def plain_input_reference(name: str, m: int) -> TransformReference:
    """Reference (b) for eqa_winograd_f{m}k5_input on the case's x (the V that the filter gradient contracts)."""
    x = inputs(name)[0].double()
    return TransformReference(input_transform(x, m), TRANSFORM_GAMMA * input_transform(x, m, absolute=True))


# ---- measures -------------------------------------------------------------------------------------------------------------

QUANTITIES = ("d_bank", "d_x:interior", "d_x:border")


def measure(got: torch.Tensor, want: torch.Tensor) -> float:
    """max |got - want| over the largest reference entry."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return ((got - want).abs().max() / want.abs().max()).item()


def border_mask(H: int, W: int) -> torch.Tensor:
    m = torch.ones(H, W, dtype=torch.bool)
    m[BORDER:H - BORDER, BORDER:W - BORDER] = False
    return m


def measure_input_gradient(got: torch.Tensor, want: torch.Tensor) -> dict:
    """{"d_x:interior", "d_x:border"}: max |got - want| over the region, each over the largest reference entry of the whole
    gradient.  The border is the outer four pixels, the ones a 5 x 5 window reaches the zero padding of dy from."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    b = border_mask(*want.shape[-2:])
    assert b.any() and (~b).any()
    diff, scale = (got - want).abs(), want.abs().max().item()
    return {"d_x:interior": diff[..., ~b].max().item() / scale, "d_x:border": diff[..., b].max().item() / scale}


def measure_transform(got: torch.Tensor, ref: TransformReference) -> float:
    """max over the entries of |got - want| / bound: at most 1 inside the a-priori bound.  Where the bound is zero (a window
    that lies in the padding) the result must be exactly zero."""
    got = got.detach().cpu().double()
    assert got.shape == ref.want.shape, (got.shape, ref.want.shape)
    diff = (got - ref.want).abs()
    ratio = torch.where(ref.bound > 0, diff / ref.bound.clamp_min(1e-300), torch.where(diff > 0, float("inf"), 0.0).double())
    return ratio.max().item()


# ---- the fp32 CPU chain's own errors, per case and tile size, and the pooled budgets -----------------------------------------


@functools.lru_cache(maxsize=None)
def cpu_chain_errors() -> dict:
    """{(quantity, case name, m): error of the fp32 CPU chain against reference (a)}; quantity "forward" as well (not budgeted:
    the forward keeps the 2e-5 of tests/test_gpu_parity.py)."""
    err = {}
    for c in CASES:
        want = reference(c.name)
        for m in tiles_of(c):
            got = chain_results(c.name, m)
            err[("forward", c.name, m)] = measure(got.y, want.y)
            err[("d_bank", c.name, m)] = measure(got.d_bank, want.d_bank)
            for k, v in measure_input_gradient(got.d_x, want.d_x).items():
                err[(k, c.name, m)] = v
    return err


@functools.lru_cache(maxsize=None)
def budgets() -> dict:
    """{quantity: M x the worst fp32 CPU chain error of that quantity over this file's cases and both tile sizes}."""
    pooled = {}
    for key, v in cpu_chain_errors().items():
        if key[0] in QUANTITIES:
            pooled[key[0]] = max(pooled.get(key[0], 0.0), v)
    return {q: M_BUDGET * v for q, v in pooled.items()}
