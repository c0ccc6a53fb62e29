"""The training kernels of ResNet18Network's basic blocks -- eqa_conv3x3_wgrad, eqa_conv3x3_dgrad (csrc/conv3x3_train.hip, conv3x3.hip)
and the eqa_bn_res_act_* family -- against fp64 evaluations of the same fp32 operands: error bounds, exactness on small integers,
adjointness, image seams, reads and writes past the end, reproducibility, refused shapes and argument checks."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3      # EQA_ERR_INVALID_ARG, EQA_ERR_UNSUPPORTED (include/eqa_hip.h)

# (N, H, W, Cin, Cout, taps, stride): the forward kernel's list (tests/test_gpu_conv3x3.py)
CASES = [
    (1, 1, 1, 64, 64, 9, 1),        # one pixel, eight taps on padding
    (1, 5, 5, 64, 64, 9, 1),        # P = 25, less than one tile
    (3, 6, 7, 64, 64, 9, 1),        # P = 126: the tile seam falls inside image 1; border pixels have memory neighbours in the next image
    (2, 5, 7, 64, 128, 9, 2),       # odd sizes at stride 2 -> 3 x 4
    (2, 6, 8, 128, 256, 9, 2),      # even sizes at stride 2: the bottom / right padding is never touched, the top / left is
    (5, 3, 3, 512, 512, 9, 1),      # the widest pair
    (2, 4, 4, 32, 96, 9, 1),        # the channel rule's small end, both column-tile widths
    (2, 4, 4, 96, 32, 9, 1),
    (17, 16, 16, 64, 64, 9, 1),     # P = 4352: more tiles than one pass of the waves over a column tile; 113 pixel ranges
    (2, 5, 7, 64, 128, 1, 2),       # the shortcut
    (2, 6, 8, 256, 512, 1, 2),
]
IDS = ["x".join(map(str, c)) for c in CASES]
SEAM = (3, 6, 7, 64, 64, 9, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _geom(H, W, taps, stride):
    k, pad = (3, 1) if taps == 9 else (1, 0)
    return k, pad, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _operands(dev, case, integers=False):
    """x, w, dz and a residual of dx's shape; `integers`: entries from {-3 .. 3}."""
    N, H, W, Cin, Cout, taps, stride = case
    g = torch.Generator(device=dev).manual_seed(1000 * Cin + Cout + 7 * N * H * W + taps + stride)
    k, _, OH, OW = _geom(H, W, taps, stride)

    def draw(*shape):
        if integers:
            return torch.randint(-3, 4, shape, device=dev, generator=g).float()
        return torch.randn(*shape, device=dev, generator=g)

    w = draw(Cout, Cin, k, k)
    return draw(N, H, W, Cin), w if integers else w / (taps * Cin) ** 0.5, draw(N, OH, OW, Cout), draw(N, H, W, Cin)


def _wgrad64(x, dz, case):
    """The contraction in fp64 without a convolution: the unfolded padded x against dz.  -> (dW, sum |x||dz|), each (Cout, Cin, k, k)."""
    N, H, W, Cin, Cout, taps, stride = case
    k, pad, OH, OW = _geom(H, W, taps, stride)
    cols = F.unfold(x.double().permute(0, 3, 1, 2), k, 1, pad, stride)                  # (N, Cin k k, OH OW)
    d = dz.double().reshape(N, OH * OW, Cout)
    return (torch.einsum("nkl,nlo->ok", cols, d).reshape(Cout, Cin, k, k), torch.einsum("nkl,nlo->ok", cols.abs(), d.abs()).reshape(Cout, Cin, k, k))


def _dgrad64(dz, w, case):
    """-> (dx, sum |dz||w|), each (N, H, W, Cin), in fp64."""
    N, H, W, Cin, Cout, taps, stride = case
    k, pad, OH, OW = _geom(H, W, taps, stride)
    out_pad = (H - ((OH - 1) * stride - 2 * pad + k), W - ((OW - 1) * stride - 2 * pad + k))

    def t(a, b):
        return F.conv_transpose2d(a.permute(0, 3, 1, 2), b, None, stride, pad, out_pad).permute(0, 2, 3, 1)

    return t(dz.double(), w.double()), t(dz.double().abs(), w.double().abs())


def _zero_bias(dev, n):
    return torch.zeros(n, device=dev)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_stays_inside_the_contraction_bound_and_is_exact_on_small_integers(dev, case):
    """Every dW entry within (P + 6) 2^-24 sum |x||dz| of the fp64 contraction of the same fp32 operands: the any-order bound of a
    P-term sum plus the fp64 combination's final rounding.  Operands from {-3 .. 3}: every partial sum is an integer below 2^24, so dW
    is the fp64 result bit for bit."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = case
    assert ops.conv3x3_wgrad_supported(*case)
    k, _, OH, OW = _geom(H, W, taps, stride)
    P = N * OH * OW
    x, _, dz, _ = _operands(dev, case)
    dW = ops.conv3x3_wgrad(x, dz, taps, stride)
    assert dW.shape == (Cout, Cin, k, k) and dW.dtype == torch.float32 and dW.is_contiguous()
    want, mag = _wgrad64(x, dz, case)
    err, bound = (dW.double() - want).abs(), (P + 6) * 2.0 ** -24 * mag
    print(f"conv3x3_wgrad {case}: largest error / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all()), (case, (err / bound.clamp_min(1e-300)).max().item())
    xi, _, dzi, _ = _operands(dev, case, integers=True)
    assert torch.equal(ops.conv3x3_wgrad(xi, dzi, taps, stride).double(), _wgrad64(xi, dzi, case)[0]), case


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad_stays_inside_the_dot_product_bound_and_is_exact_on_small_integers(dev, case):
    """Every dx entry within (taps Cout + 3) 2^-24 (sum |dz||w| + |res|) of the fp64 evaluation, with and without res; every element
    is written (the output starts as NaN-free only if it is).  Exact on operands from {-3 .. 3}."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = case
    assert ops.conv3x3_dgrad_supported(*case)
    _, w, dz, res = _operands(dev, case)
    wd = ops.pack_conv3x3_dgrad_weights(w)
    want, mag = _dgrad64(dz, w, case)
    for r in (None, res):
        dx = ops.conv3x3_dgrad(dz, wd, (H, W), r, taps, stride)
        assert dx.shape == (N, H, W, Cin) and dx.is_contiguous() and bool(torch.isfinite(dx).all())
        add = 0.0 if r is None else r.double()
        err = (dx.double() - (want + add)).abs()
        bound = (taps * Cout + 3) * 2.0 ** -24 * (mag + (0.0 if r is None else r.double().abs()))
        print(f"conv3x3_dgrad {case} res={r is not None}: largest error / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), (case, r is not None)
    _, wi, dzi, ri = _operands(dev, case, integers=True)
    got = ops.conv3x3_dgrad(dzi, ops.pack_conv3x3_dgrad_weights(wi), (H, W), ri, taps, stride)
    assert torch.equal(got.double(), _dgrad64(dzi, wi, case)[0] + ri.double()), case


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_three_kernels_are_adjoint(dev, case):
    """<dz, conv(x)>, <dgrad(dz), x> and <wgrad(x, dz), w>, summed in fp64 from the kernels' outputs, agree to 1e-4 (|rhs| + 1)."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = case
    x, w, dz, _ = _operands(dev, case)
    z = ops.conv3x3_nhwc(x, ops.pack_conv3x3_weights(w), _zero_bias(dev, Cout), None, False, taps, stride)
    a = (dz.double() * z.double()).sum().item()
    b = (ops.conv3x3_dgrad(dz, ops.pack_conv3x3_dgrad_weights(w), (H, W), None, taps, stride).double() * x.double()).sum().item()
    c = (ops.conv3x3_wgrad(x, dz, taps, stride).double() * w.double()).sum().item()
    print(f"adjointness {case}: {a:.9e} {b:.9e} {c:.9e}")
    assert abs(b - a) <= 1e-4 * (abs(a) + 1) and abs(c - a) <= 1e-4 * (abs(a) + 1), (a, b, c)


def test_nothing_leaks_across_an_image_seam(dev):
    """(3, 6, 7).  Filter gradient: x of images 0 and 2 filled with a large constant, their dz zero; dW equals what a batch of image
    1 alone gives, bit for bit -- image 1 holds small integers, so that every order of summation gives the same bits and only a
    neighbour read across the seam (1e6 times a border pixel's dz) can make a difference.  Data gradient: dz of images 0 and 2 large;
    dx of image 1 equals the batch of image 1 alone bit for bit (a pixel's chain does not depend on its tile)."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = SEAM
    x, _, dz, _ = _operands(dev, SEAM, integers=True)
    x[0] = x[2] = 1.0e6
    dz[0] = dz[2] = 0.0
    whole = ops.conv3x3_wgrad(x, dz)
    alone = ops.conv3x3_wgrad(x[1:2].contiguous(), dz[1:2].contiguous())
    assert torch.equal(whole, alone) and bool(whole.abs().max() > 0)
    _, w, dz, res = _operands(dev, SEAM)
    dz[0] = dz[2] = 1.0e6
    wd = ops.pack_conv3x3_dgrad_weights(w)
    for r in (None, res):
        whole = ops.conv3x3_dgrad(dz, wd, (H, W), r)
        alone = ops.conv3x3_dgrad(dz[1:2].contiguous(), wd, (H, W), None if r is None else r[1:2].contiguous())
        assert torch.equal(whole[1:2], alone), r is not None


def _framed(t, fill, band=96):
    """t as an interior view of a larger buffer filled with `fill`: (buffer, view); the view's pointer stays 16-byte aligned."""
    buf = torch.full((t.numel() + 2 * band,), fill, device=t.device, dtype=t.dtype)
    view = buf[band:band + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("case", [(1, 5, 5, 64, 64, 9, 1), SEAM, (2, 5, 7, 64, 128, 9, 2), (2, 5, 7, 64, 128, 1, 2), (2, 4, 4, 32, 96, 9, 1)],
                         ids=lambda c: "x".join(map(str, c)))
def test_nothing_past_the_end_is_read_or_written(dev, case):
    """x, dz and res inside buffers of NaN, dW and dx inside buffers of a sentinel: the results hold no NaN, equal the plain calls,
    and the sentinels are intact."""
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    N, H, W, Cin, Cout, taps, stride = case
    k, _, OH, OW = _geom(H, W, taps, stride)
    x, w, dz, res = _operands(dev, case)
    wd = ops.pack_conv3x3_dgrad_weights(w)
    nan = float("nan")
    (_, xv), (_, dzv), (_, rv) = _framed(x, nan), _framed(dz, nan), _framed(res, nan)
    band = 96
    dWb, dWv = _framed(torch.zeros(Cout, Cin, k, k, device=dev), 7.0)
    dxb, dxv = _framed(torch.zeros(N, H, W, Cin, device=dev), 7.0)
    work = torch.empty(max(lib.eqa_conv3x3_wgrad_workspace_bytes(*case) // 4, 4), device=dev)
    assert lib.eqa_conv3x3_wgrad(xv.data_ptr(), dzv.data_ptr(), work.data_ptr(), dWv.data_ptr(), *case, None) == 0
    assert lib.eqa_conv3x3_dgrad(dzv.data_ptr(), wd.data_ptr(), rv.data_ptr(), dxv.data_ptr(), *case, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dWv, ops.conv3x3_wgrad(x, dz, taps, stride)) and torch.equal(dxv, ops.conv3x3_dgrad(dz, wd, (H, W), res, taps, stride))
    for buf in (dWb, dxb):
        assert bool((buf[:band] == 7.0).all()) and bool((buf[-band:] == 7.0).all()), "written outside the result"


def test_two_launches_give_the_same_bits(dev):
    from equiadapt_amd import ops

    for case in ((17, 16, 16, 64, 64, 9, 1), (2, 6, 8, 128, 256, 9, 2), (2, 6, 8, 256, 512, 1, 2), (5, 3, 3, 512, 512, 9, 1)):
        N, H, W, Cin, Cout, taps, stride = case
        x, w, dz, res = _operands(dev, case)
        wd = ops.pack_conv3x3_dgrad_weights(w)
        assert torch.equal(ops.conv3x3_wgrad(x, dz, taps, stride), ops.conv3x3_wgrad(x, dz, taps, stride)), case
        assert torch.equal(ops.conv3x3_dgrad(dz, wd, (H, W), res, taps, stride), ops.conv3x3_dgrad(dz, wd, (H, W), res, taps, stride)), case


def test_queries_and_launches_agree_on_refused_shapes_and_the_argument_checks(dev):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    ok = (2, 4, 4, 64, 64, 9, 1)
    # p: x, dz or dx (2048 floats); q: another of them; r: the workspace; s: dW or the packed filters (36864 floats)
    bufs = [torch.zeros(n, device=dev) for n in (2048, 2048, lib.eqa_conv3x3_wgrad_workspace_bytes(*ok) // 4, 9 * 64 * 64)]
    p, q, r, s = (b.data_ptr() for b in bufs)
    for shape in ((2, 4, 4, 48, 64, 9, 1), (2, 4, 4, 64, 544, 9, 1), (2, 4, 4, 64, 64, 1, 1)):
        assert not ops.conv3x3_wgrad_supported(*shape) and not ops.conv3x3_dgrad_supported(*shape)
        assert lib.eqa_conv3x3_wgrad(p, q, r, s, *shape, None) == UNSUPPORTED
        assert lib.eqa_conv3x3_dgrad(p, q, None, s, *shape, None) == UNSUPPORTED
    with pytest.raises(_lib.EqaLibraryError):
        ops.conv3x3_wgrad(torch.zeros(2, 4, 4, 48, device=dev), torch.zeros(2, 4, 4, 64, device=dev))
    assert lib.eqa_conv3x3_wgrad(p, q, r, s, *ok, None) == 0
    assert lib.eqa_conv3x3_dgrad(p, s, None, q, *ok, None) == 0
    for bad in ((p + 4, q, r, s), (p, q + 8, r, s), (p, q, r + 4, s), (p, q, r, s + 4)):
        assert lib.eqa_conv3x3_wgrad(*bad, *ok, None) == UNSUPPORTED                # misaligned
    for bad in ((p + 4, s, None, q), (p, s + 4, None, q), (p, s, r + 4, q), (p, s, None, q + 8)):
        assert lib.eqa_conv3x3_dgrad(*bad, *ok, None) == UNSUPPORTED
    for bad in ((p, p, r, s), (p, q, p, s), (p, q, r, p), (p, q, r, q), (p, q, s, s), (None, q, r, s), (p, q, None, s), (p, q, r, None)):
        assert lib.eqa_conv3x3_wgrad(*bad, *ok, None) == INVALID                    # equal base pointers, NULL
    for bad in ((p, s, None, p), (p, s, q, q), (None, s, None, q), (p, None, None, q), (p, s, None, None)):
        assert lib.eqa_conv3x3_dgrad(*bad, *ok, None) == INVALID
    dW = torch.full((64, 64, 3, 3), 5.0, device=dev)
    assert lib.eqa_conv3x3_wgrad(None, None, None, dW.data_ptr(), 0, 4, 4, 64, 64, 9, 1, None) == 0
    torch.cuda.synchronize()
    assert bool((dW == 0).all()), "N = 0 zeroes dW"


def _bn_case(npix, C, form, seed):
    """z, res, gamma, beta, gy on the CPU for one form; with a ReLU no t = bn(z) + res lies within 1e-4 of 0 (entries that did were
    redrawn, fewer than 1 % of them), so a mask flip cannot hide a real error."""
    has_res, relu = form
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(npix, C, generator=g) * 1.5 + 0.3
    res = torch.randn(npix, C, generator=g) if has_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    gy = torch.randn(npix, C, generator=g)

    def t64():
        t = F.batch_norm(z.double(), None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)
        return t + res.double() if has_res else t

    if relu:
        near = t64().abs() < 1e-4
        assert near.float().mean().item() < 0.01
        for _ in range(8):
            if not bool(near.any()):
                break
            z[near] = torch.randn(int(near.sum()), generator=g) * 1.5 + 0.3
            if has_res:
                res[near] = torch.randn(int(near.sum()), generator=g)
            near = t64().abs() < 1e-4
        assert not bool(near.any())
    return z, res, gamma, beta, gy


@pytest.mark.parametrize("form", [(False, True), (True, True), (False, False)], ids=["relu(bn)", "relu(bn+res)", "bn"])
@pytest.mark.parametrize("npix,C", [(25, 64), (126, 128), (1030, 512)])
def test_bn_res_act_forward_and_backward_match_autograd(dev, npix, C, form):
    """The three forms of a basic block against fp64 autograd through F.batch_norm(training=True) + res + relu, at the tolerances of
    test_bn_act_forward_and_backward_match_autograd; dres is gy [y > 0] bit for bit."""
    from equiadapt_amd import ops

    has_res, relu = form
    z, res, gamma, beta, gy = _bn_case(npix, C, form, 100 * C + npix + 2 * has_res + relu)
    z64, g64, b64 = z.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if has_res else None
    t = F.batch_norm(z64, None, None, g64, b64, True, 0.1, 1e-5)
    if has_res:
        t = t + r64
    y64 = F.relu(t) if relu else t
    (y64 * gy.double()).sum().backward()
    zd, gyd = z.to(dev), gy.to(dev)
    rd = res.to(dev) if has_res else None
    mean, var = ops.bn_batch_stats(zd)
    rstd = torch.rsqrt(var + 1e-5)
    scale = (gamma.to(dev).double() * rstd).float().contiguous()
    shift = (beta.to(dev).double() - mean * gamma.to(dev).double() * rstd).float().contiguous()
    y = ops.bn_res_act_fwd(zd, scale, shift, rd, relu)
    assert (y.cpu().double() - y64.detach()).abs().max().item() <= 1e-5
    dz, dgamma, dbeta, dres = ops.bn_res_act_bwd(gyd, zd, scale, shift, mean.float().contiguous(), rstd.float().contiguous(), gamma.to(dev), rd,
                                                 relu, need_dres=has_res)
    sc = z64.grad.abs().max().item()
    assert (dz.cpu().double() - z64.grad).abs().max().item() <= 2e-5 * sc + 1e-6
    assert (dgamma.cpu().double() - g64.grad).abs().max().item() <= 2e-5 * g64.grad.abs().max().item() + 1e-5
    assert (dbeta.cpu().double() - b64.grad).abs().max().item() <= 2e-5 * b64.grad.abs().max().item() + 1e-5
    if has_res:
        assert torch.equal(dres, torch.where(y > 0, gyd, torch.zeros_like(gyd)))
        assert torch.equal(dres.cpu().double(), r64.grad)
    else:
        assert dres is None


def test_conv3x3_function_against_fp64_autograd(dev):
    """Conv3x3Function at P = 126 against fp64 autograd through F.conv2d: the output and both gradients inside the kernels' bounds,
    with each gradient on the kernel and on the library, and a branch gradient handed over through the data gradient's res."""
    from equiadapt_amd.images.canonicalization_networks.custom_nonequivariant_networks import Conv3x3Function, _BranchGrad

    N, H, W, Cin, Cout, taps, stride = SEAM
    P = N * H * W
    x, w, gz, other = _operands(dev, SEAM)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z64 = F.conv2d(x64.permute(0, 3, 1, 2), w64, None, 1, 1).permute(0, 2, 3, 1)
    (z64 * gz.double()).sum().backward()
    _, mag_w = _wgrad64(x, gz, SEAM)
    _, mag_x = _dgrad64(gz, w, SEAM)
    mag_z = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w.double().abs(), None, 1, 1).permute(0, 2, 3, 1)
    for wgrad_kernel, dgrad_kernel, branch in ((True, True, False), (False, False, False), (True, True, True), (True, False, True)):
        xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        hint = _BranchGrad() if branch else None
        z = Conv3x3Function.apply(xs, ws, taps, stride, _zero_bias(dev, Cout), wgrad_kernel, dgrad_kernel, hint)
        assert bool(((z.double() - z64.detach()).abs() <= (taps * Cin + 3) * 2.0 ** -24 * mag_z).all())
        if branch:
            hint.give(other)
        (z * gz).sum().backward()
        add = other.double() if branch else 0.0
        if dgrad_kernel:
            assert bool(((xs.grad.double() - (x64.grad + add)).abs() <= (taps * Cout + 3) * 2.0 ** -24 * (mag_x + (other.double().abs() if branch else 0.0))).all())
        else:
            assert (xs.grad.double() - (x64.grad + add)).abs().max().item() <= 1e-4 * (x64.grad + add).abs().max().item()
        if wgrad_kernel:
            assert bool(((ws.grad.double() - w64.grad).abs() <= (P + 6) * 2.0 ** -24 * mag_w).all())
        else:
            assert (ws.grad.double() - w64.grad).abs().max().item() <= 1e-4 * w64.grad.abs().max().item()    # (the library's algorithm is its own)
