"""eqa_convwide_nhwc (csrc/conv_wide.hip), the split-K convolution of the wide ResNets' bottlenecks: bit equality with
eqa_conv3x3_nhwc and eqa_gconv1x1_nhwc at ksplit 1, exact integer results at every admitted ksplit (a stage dropped or doubled at a
slice seam shows there), the project's fp64 dot-product bound, image seams, rows past the pixel count in y and in the workspace,
reproducibility, the library's own choice of ksplit, return codes."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3      # EQA_ERR_INVALID_ARG, EQA_ERR_UNSUPPORTED (include/eqa_hip.h)

# (N, H, W, Cin, Cout, taps, stride)
WIDE = [
    (1, 3, 3, 1024, 64, 9, 1),      # layer4's K loop: T / 2 = 288
    (1, 3, 3, 544, 32, 9, 2),       # OH = 2, a 32-wide column tile, an odd Cin / 32: T / 2 = 153, which 2, 5 and 16 do not divide
    (2, 3, 3, 2048, 64, 1, 1),      # P = 18; the widest input
    (1, 2, 2, 32, 2048, 1, 1),      # T / 2 = 1: only ksplit 1; the widest output
    (1, 3, 3, 1024, 2048, 1, 2),    # layer4's projection
]
SPLITS = (1, 2, 3, 5, 16)


def _id(c):
    return "x".join(map(str, c))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _geom(H, W, taps, stride):
    k, pad = (3, 1) if taps == 9 else (1, 0)
    return k, pad, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _splits(case):
    half = case[5] * case[3] // 32                       # T / 2
    return sorted({k for k in SPLITS + (min(16, half),) if k <= min(16, half)})


def _operands(dev, N, H, W, Cin, Cout, taps, stride, integers=False):
    g = torch.Generator(device=dev).manual_seed(1000 * Cin + Cout + 7 * N * H * W + taps + stride)
    k, _, OH, OW = _geom(H, W, taps, stride)

    def rn(*shape):
        if integers:
            return torch.randint(-2, 3, shape, device=dev, generator=g).float()
        return torch.randn(*shape, device=dev, generator=g)

    w = rn(Cout, Cin, k, k)
    return rn(N, H, W, Cin), w if integers else w / (taps * Cin) ** 0.5, rn(Cout), rn(N, OH, OW, Cout)


@pytest.mark.parametrize("case,has_res,relu", [((2, 5, 7, 32, 64, 9, 1), True, True), ((2, 5, 7, 64, 32, 9, 2), False, False),
                                               ((3, 4, 4, 64, 96, 1, 2), False, False), ((2, 6, 7, 128, 128, 9, 1), True, False)],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else str(int(v)))
def test_ksplit_one_is_conv3x3_bit_for_bit(dev, case, has_res, relu):
    from equiadapt_amd import ops

    assert ops.conv3x3_supported(*case) and ops.convwide_supported(*case)
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    want = ops.conv3x3_nhwc(x, wpk, bias, res if has_res else None, relu, case[5], case[6])
    got = ops.convwide_nhwc(x, wpk, bias, res if has_res else None, relu, case[5], case[6], ksplit=1)
    assert torch.equal(got, want)


def test_one_by_one_at_stride_one_is_gconv1x1_bit_for_bit(dev):
    """eqa_gconv1x1_nhwc without its scale / shift pair runs the same chains -- stages ascending, one accumulator per output, bias then
    res then ReLU -- so the new 1 x 1 stride-1 form at ksplit 1 is held to its bits, not to the fp64 bound."""
    from equiadapt_amd import ops

    for case, has_res, relu in (((2, 5, 7, 64, 96, 1, 1), True, True), ((3, 4, 4, 512, 128, 1, 1), False, False)):
        N, H, W, Cin, Cout = case[:5]
        assert ops.gconv1x1_supported(N * H * W, Cin, Cout) and ops.convwide_supported(*case)
        x, w, bias, res = _operands(dev, *case)
        want = ops.gconv1x1_nhwc(x.view(-1, Cin), ops.pack_gconv1x1_weights(w), bias, res.view(-1, Cout) if has_res else None, relu=relu)
        got = ops.convwide_nhwc(x, ops.pack_conv3x3_weights(w), bias, res if has_res else None, relu, 1, 1, ksplit=1)
        assert torch.equal(got.view(-1, Cout), want), case


@pytest.mark.parametrize("case", WIDE, ids=_id)
def test_integer_operands_are_exact_at_every_split(dev, case):
    """x and w in {-2 .. 2}, bias and res integer: every partial and every sum is an integer below 4 * 9216 + 4 < 2^24, exact in
    fp32 whatever the order, so the output IS the integer result: a stage dropped or doubled at a slice seam cannot hide."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = case
    k, pad, OH, OW = _geom(H, W, taps, stride)
    x, w, bias, res = _operands(dev, *case, integers=True)
    wpk = ops.pack_conv3x3_weights(w)
    dot = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride, pad).permute(0, 2, 3, 1)
    splits = _splits(case)
    assert splits[0] == 1 and (case[3] != 32 or splits == [1])
    for ks in splits:
        for has_res, relu in ((True, True), (False, False)):
            want = dot + (res.double() if has_res else 0.0)
            if relu:
                want = want.clamp_min(0.0)
            y = ops.convwide_nhwc(x, wpk, bias, res if has_res else None, relu, taps, stride, ksplit=ks)
            assert y.shape == (N, OH, OW, Cout) and y.dtype == torch.float32 and y.is_contiguous()
            assert torch.equal(y.double(), want), (case, ks, has_res, relu, (y.double() - want).abs().max().item())
    if Cin == 544:
        assert all((taps * Cin // 32) % ks for ks in (2, 5, 16)) and {2, 5, 16} <= set(splits)     # splits that do not divide T / 2


@pytest.mark.parametrize("case", WIDE, ids=_id)
def test_every_split_stays_inside_the_dot_product_bound(dev, case):
    """Every output within (taps Cin + 3) 2^-24 (sum |x||w| + |bias| + |res|) of the fp64 evaluation of the same fp32 operands -- the
    project's bound for the unsplit chain: a split only shortens the chains, and the partials are added in fp64.  Measured largest
    error / bound: 0.0002, 0.0003, 0.0013, 0.109 (32 -> 2048: the bound has 35 terms there, not thousands) and 0.0029."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = case
    k, pad, OH, OW = _geom(H, W, taps, stride)
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    xd = x.double().permute(0, 3, 1, 2)
    dot = F.conv2d(xd, w.double(), None, stride, pad).permute(0, 2, 3, 1)
    mag = F.conv2d(xd.abs(), w.double().abs(), None, stride, pad).permute(0, 2, 3, 1)
    worst = 0.0
    for ks in _splits(case):
        for has_res, relu in itertools.product((False, True), repeat=2):
            y = ops.convwide_nhwc(x, wpk, bias, res if has_res else None, relu, taps, stride, ksplit=ks)
            want = dot + bias.double() + (res.double() if has_res else 0.0)
            bound = (taps * Cin + 3) * 2.0 ** -24 * (mag + bias.double().abs() + (res.double().abs() if has_res else 0.0))
            if relu:
                want = want.clamp_min(0.0)
            err = (y.double() - want).abs()
            worst = max(worst, (err / bound).max().item())
            assert bool((err <= bound).all()), (case, ks, has_res, relu, (err / bound).max().item())
    print(f"convwide {case}: largest error / bound over splits {_splits(case)} and the four forms = {worst:.4f}")


def test_nothing_leaks_across_an_image_seam(dev):
    """Three 3 x 3 images at taps 9: one 64-row tile spans all three, and a border pixel's neighbour in memory belongs to the adjacent
    image.  At ksplit 1 and 4 the batch equals the three per-image calls bit for bit."""
    from equiadapt_amd import ops

    case = (3, 3, 3, 128, 64, 9, 1)
    x, w, bias, res = _operands(dev, *case)
    x = x.clone()
    x[0] = 1.0e6
    x[2] = -1.0e6
    wpk = ops.pack_conv3x3_weights(w)
    for ks in (1, 4):
        whole = ops.convwide_nhwc(x, wpk, bias, res, True, 9, 1, ksplit=ks)
        for n in range(3):
            alone = ops.convwide_nhwc(x[n:n + 1].contiguous(), wpk, bias, res[n:n + 1].contiguous(), True, 9, 1, ksplit=ks)
            assert torch.equal(whole[n:n + 1], alone), (ks, n)


@pytest.mark.parametrize("case,ks", [((2, 5, 7, 64, 128, 9, 2), 1), ((2, 5, 7, 64, 128, 9, 2), 5), ((2, 3, 3, 2048, 64, 1, 1), 16),
                                     ((3, 5, 5, 96, 96, 9, 1), 3)], ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_rows_past_the_pixel_count_are_never_stored(dev, case, ks):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    N, H, W, Cin, Cout, taps, stride = case
    _, _, OH, OW = _geom(H, W, taps, stride)
    P = N * OH * OW
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    want = ops.convwide_nhwc(x, wpk, bias, res, True, taps, stride, ksplit=ks)
    big_x = torch.cat([x.reshape(-1, Cin), torch.full((70, Cin), 3.0, device=dev)])   # (what lies behind the map must not be read into it)
    big_r = torch.cat([res.reshape(P, Cout), torch.full((70, Cout), 5.0, device=dev)])
    y = torch.full((P + 70, Cout), 7.0, device=dev)
    work = torch.full((ks * P + 70, Cout), 9.0, device=dev)
    assert lib.eqa_convwide_workspace_bytes(*case, ks) == (0 if ks == 1 else ks * P * Cout * 4)
    st = lib.eqa_convwide_nhwc(big_x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), big_r.data_ptr(), 1, y.data_ptr(), work.data_ptr(), N, H, W,
                               Cin, Cout, taps, stride, ks, None)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:P], want.reshape(P, Cout))
    assert bool((y[P:] == 7.0).all()), "rows beyond the pixel count must not be written"
    written = ks * P if ks > 1 else 0
    assert bool((work[written:] == 9.0).all()), "the workspace is written up to ksplit * P rows and no further"
    if ks > 1:
        # the slices in fp64, in index order, rounded once: the reduction's own rule, from the partials it was given
        part = work[:written].view(ks, P, Cout).double()
        acc = torch.zeros(P, Cout, dtype=torch.float64, device=dev)
        for i in range(ks):
            acc += part[i]
        z = (acc.float() + bias) + res.reshape(P, Cout)
        assert torch.equal(y[:P], z.clamp_min(0.0))


def test_two_launches_give_the_same_bits_and_zero_means_the_library_choice(dev):
    from equiadapt_amd import ops

    for case in WIDE + [(5, 6, 6, 256, 256, 9, 1)]:
        x, w, bias, res = _operands(dev, *case)
        wpk = ops.pack_conv3x3_weights(w)
        ks = ops.convwide_ksplit(*case)
        assert 1 <= ks <= min(16, case[5] * case[3] // 32)
        a = ops.convwide_nhwc(x, wpk, bias, res, True, case[5], case[6], ksplit=ks)
        b = ops.convwide_nhwc(x, wpk, bias, res, True, case[5], case[6], ksplit=ks)
        c = ops.convwide_nhwc(x, wpk, bias, res, True, case[5], case[6])
        assert torch.equal(a, b) and torch.equal(a, c), case
    assert ops.convwide_ksplit(1, 3, 3, 1024, 64, 9, 1) == 16 and ops.convwide_ksplit(1, 2, 2, 32, 2048, 1, 1) == 1


def test_return_codes(dev):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    case = (2, 4, 4, 64, 64, 9, 1)
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    y = torch.empty(2, 4, 4, 64, device=dev)
    work = torch.empty(4 * y.numel(), device=dev)
    px, pw, pb, pr, py, pk = (t.data_ptr() for t in (x, wpk, bias, res, y, work))

    def call(px=px, pw=pw, pb=pb, pr=pr, py=py, pk=pk, n=2, cin=64, taps=9, stride=1, ks=4):
        return lib.eqa_convwide_nhwc(px, pw, pb, pr, 0, py, pk, n, 4, 4, cin, 64, taps, stride, ks, None)

    assert call() == 0 and call(ks=1, pk=None) == 0 and call(ks=0) == 0 and call(pr=None) == 0
    assert call(n=0) == 0 and call(n=0, px=None, py=None, pk=None) == 0           # N = 0 launches nothing
    assert call(cin=2080) == UNSUPPORTED and call(taps=4) == UNSUPPORTED and call(stride=3) == UNSUPPORTED
    assert call(ks=17) == UNSUPPORTED and call(ks=-1) == UNSUPPORTED and call(taps=1, ks=3) == UNSUPPORTED
    assert call(px=None) == INVALID and call(pw=None) == INVALID and call(pb=None) == INVALID and call(py=None) == INVALID
    assert call(pk=None) == INVALID                                                 # NULL workspace with ksplit > 1
    assert call(py=px) == INVALID and call(py=pr) == INVALID
    for alias in (px, pw, pb, pr, py):
        assert call(pk=alias) == INVALID
    assert call(px=px + 4) == UNSUPPORTED and call(pb=pb + 8) == UNSUPPORTED and call(pr=pr + 4) == UNSUPPORTED and call(pk=pk + 4) == UNSUPPORTED
    torch.cuda.synchronize()
    with pytest.raises(_lib.EqaLibraryError):
        ops.convwide_nhwc(x, wpk, bias, None, False, 9, 3)
    with pytest.raises(_lib.EqaLibraryError):
        ops.convwide_nhwc(x, wpk, bias, None, False, 9, 1, ksplit=17)
    with pytest.raises(RuntimeError):
        ops.convwide_nhwc(x.permute(0, 3, 1, 2), wpk, bias, None, False, 9, 1)      # not (N, H, W, C)
