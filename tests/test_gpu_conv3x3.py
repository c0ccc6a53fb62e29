"""eqa_conv3x3_nhwc (csrc/conv3x3.hip), the fused 3 x 3 / 1 x 1-stride-2 convolution of ResNet18Network's blocks, against the fp64
evaluation of the same fp32 operands: error bound, image seams, rows past the pixel count, reproducibility, refused shapes."""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3      # EQA_ERR_UNSUPPORTED (include/eqa_hip.h)

# (N, H, W, Cin, Cout, taps, stride)
CASES = [
    (1, 1, 1, 64, 64, 9, 1),        # one pixel, eight taps on padding
    (1, 5, 5, 64, 64, 9, 1),        # P = 25, less than one tile
    (3, 6, 7, 64, 64, 9, 1),        # P = 126: the tile seam falls inside image 1; border pixels have memory neighbours in the next image
    (2, 5, 7, 64, 128, 9, 2),       # odd sizes at stride 2 -> 3 x 4
    (2, 6, 8, 128, 256, 9, 2),      # even sizes at stride 2: the bottom / right padding is never touched, the top / left is
    (5, 3, 3, 512, 512, 9, 1),      # the widest pair
    (2, 4, 4, 32, 96, 9, 1),        # the channel rule's small end, both column-tile widths
    (2, 4, 4, 96, 32, 9, 1),
    (17, 16, 16, 64, 64, 9, 1),     # P = 4352: more tiles than one pass of the waves over a column tile
    (2, 5, 7, 64, 128, 1, 2),       # the shortcut
    (2, 6, 8, 256, 512, 1, 2),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _geom(H, W, taps, stride):
    k, pad = (3, 1) if taps == 9 else (1, 0)
    return k, pad, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _operands(dev, N, H, W, Cin, Cout, taps, stride):
    g = torch.Generator(device=dev).manual_seed(1000 * Cin + Cout + 7 * N * H * W + taps + stride)
    k, _, OH, OW = _geom(H, W, taps, stride)

    def rn(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    return rn(N, H, W, Cin), rn(Cout, Cin, k, k) / (taps * Cin) ** 0.5, rn(Cout), rn(N, OH, OW, Cout)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_stays_inside_the_dot_product_bound(dev, case):
    """Every output within (taps Cin + 3) 2^-24 (sum |x||w| + |bias| + |res|) of the fp64 evaluation (F.conv2d in double on the NCHW
    view) of the same fp32 operands: the any-order bound of a taps Cin-term dot product plus the bias, the residual and their
    roundings (ReLU is 1-Lipschitz).  Every combination of residual and ReLU."""
    from equiadapt_amd import ops

    N, H, W, Cin, Cout, taps, stride = case
    assert ops.conv3x3_supported(*case)
    k, pad, OH, OW = _geom(H, W, taps, stride)
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    assert wpk.shape == (taps, Cin // 16, Cout // 32, 2, 64, 4)
    xd = x.double().permute(0, 3, 1, 2)
    dot = F.conv2d(xd, w.double(), None, stride, pad).permute(0, 2, 3, 1)
    mag = F.conv2d(xd.abs(), w.double().abs(), None, stride, pad).permute(0, 2, 3, 1)
    worst = 0.0
    for has_res, relu in itertools.product((False, True), repeat=2):
        y = ops.conv3x3_nhwc(x, wpk, bias, res if has_res else None, relu, taps, stride)
        assert y.shape == (N, OH, OW, Cout) and y.dtype == torch.float32 and y.is_contiguous()
        want = dot + bias.double() + (res.double() if has_res else 0.0)
        bound = (taps * Cin + 3) * 2.0 ** -24 * (mag + bias.double().abs() + (res.double().abs() if has_res else 0.0))
        if relu:
            want = want.clamp_min(0.0)
        err = (y.double() - want).abs()
        worst = max(worst, (err / bound).max().item())
        assert bool((err <= bound).all()), (case, has_res, relu, (err / bound).max().item())
        if relu:
            assert y.min().item() >= 0.0
    print(f"conv3x3 {case}: largest error / bound over the four forms = {worst:.3f}")


def test_nothing_leaks_across_an_image_seam(dev):
    """(3, 6, 7): images 0 and 2 filled with a large constant; image 1's output equals, bit for bit, what a batch of image 1 alone
    gives -- a border pixel's neighbour in memory belongs to the adjacent image and must load as padding."""
    from equiadapt_amd import ops

    case = (3, 6, 7, 64, 64, 9, 1)
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    x = x.clone()
    x[0] = 1.0e6
    x[2] = 1.0e6
    for has_res, relu in itertools.product((False, True), repeat=2):
        whole = ops.conv3x3_nhwc(x, wpk, bias, res if has_res else None, relu)
        alone = ops.conv3x3_nhwc(x[1:2].contiguous(), wpk, bias, res[1:2].contiguous() if has_res else None, relu)
        assert torch.equal(whole[1:2], alone), (has_res, relu)


@pytest.mark.parametrize("case", [(1, 5, 5, 64, 64, 9, 1), (3, 6, 7, 64, 64, 9, 1), (2, 5, 7, 64, 128, 9, 2), (2, 5, 7, 64, 128, 1, 2)],
                         ids=lambda c: "x".join(map(str, c)))
def test_rows_past_the_pixel_count_are_never_stored(dev, case):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    N, H, W, Cin, Cout, taps, stride = case
    _, _, OH, OW = _geom(H, W, taps, stride)
    P = N * OH * OW
    x, w, bias, res = _operands(dev, *case)
    wpk = ops.pack_conv3x3_weights(w)
    want = ops.conv3x3_nhwc(x, wpk, bias, res, True, taps, stride)
    big_x = torch.cat([x.reshape(-1, Cin), torch.full((70, Cin), 3.0, device=dev)])   # (what lies behind the map must not be read into it)
    big_r = torch.cat([res.reshape(P, Cout), torch.full((70, Cout), 5.0, device=dev)])
    y = torch.full((P + 70, Cout), 7.0, device=dev)
    st = lib.eqa_conv3x3_nhwc(big_x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), big_r.data_ptr(), 1, y.data_ptr(), N, H, W, Cin, Cout, taps,
                              stride, None)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:P], want.reshape(P, Cout))
    assert bool((y[P:] == 7.0).all()), "rows beyond the pixel count must not be written"


def test_two_launches_give_the_same_bits(dev):
    from equiadapt_amd import ops

    for case in ((17, 16, 16, 64, 64, 9, 1), (2, 6, 8, 128, 256, 9, 2), (2, 6, 8, 256, 512, 1, 2)):
        x, w, bias, res = _operands(dev, *case)
        wpk = ops.pack_conv3x3_weights(w)
        a = ops.conv3x3_nhwc(x, wpk, bias, res, True, case[5], case[6])
        b = ops.conv3x3_nhwc(x, wpk, bias, res, True, case[5], case[6])
        assert torch.equal(a, b), case


def test_refused_shapes_raise_and_misaligned_pointers_are_unsupported(dev):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    x, w, bias, res = _operands(dev, 2, 4, 4, 64, 64, 1, 2)
    wpk1 = ops.pack_conv3x3_weights(w)
    with pytest.raises(_lib.EqaLibraryError):
        ops.conv3x3_nhwc(x, wpk1, bias, None, False, 1, 1)                      # the 1 x 1 form is the stride-2 shortcut only
    with pytest.raises(_lib.EqaLibraryError):
        ops.conv3x3_nhwc(x, ops.pack_conv3x3_weights(torch.randn(64, 64, 3, 3, device=dev)), bias, None, False, 9, 3)
    with pytest.raises(RuntimeError):
        ops.conv3x3_nhwc(x.permute(0, 3, 1, 2), wpk1, bias, None, False, 1, 2)  # not (N, H, W, C)
    with pytest.raises(RuntimeError):
        ops.conv3x3_nhwc(x.cpu(), wpk1, bias, None, False, 1, 2)
    y = torch.empty(2, 2, 2, 64, device=dev)
    args = (0, y.data_ptr(), 2, 4, 4, 64, 64, 1, 2, None)
    assert lib.eqa_conv3x3_nhwc(x.data_ptr(), wpk1.data_ptr(), bias.data_ptr(), None, *args) == 0
    assert lib.eqa_conv3x3_nhwc(x.data_ptr() + 4, wpk1.data_ptr(), bias.data_ptr(), None, *args) == UNSUPPORTED
    assert lib.eqa_conv3x3_nhwc(x.data_ptr(), wpk1.data_ptr(), bias.data_ptr() + 8, None, *args) == UNSUPPORTED
    assert lib.eqa_conv3x3_nhwc(x.data_ptr(), wpk1.data_ptr(), bias.data_ptr(), res.data_ptr() + 4, *args) == UNSUPPORTED
    torch.cuda.synchronize()
