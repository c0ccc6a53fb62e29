"""eqa_crop_resize_aa_nhwc: the staged resize kernel writing pixels (B, OH, OW, C) and one |y| maximum per block.

Every pixel must carry the bits eqa_crop_resize_aa gives it (same taps, weights and order of the two passes), and the maximum over
the slots must BE max |y| -- the fused lifting kernel scales its pixels by it.  What can go wrong in a kernel that walks the planes
of an image and keeps their results in registers: a plane stored at another plane's position or another band's, a prefetch that runs
past the image it belongs to (the next image of the block is img + step, not img + 1), a trip of the register run dropped at a band
that is not full (OH % band != 0), a block without an image that leaves its slot unwritten.  The shapes: the headline's (K = 5,
16-row bands, 96 % 16 == 0), the reference tutorial's up-sampling (three taps, 8-row bands), one channel, and a map with fewer bands
than a group of eight blocks along x, whose last band is ragged only where OH % 8 != 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# (B, C, H, W), crop, out
SHAPES = [((2, 3, 224, 224), 180, 96), ((5, 3, 64, 64), 58, 64), ((3, 1, 224, 224), 180, 96), ((1, 3, 40, 40), 32, 24)]


def _tables(shape, crop, out, dev):
    from equiadapt_amd.images import geometry

    t = geometry.aa_resize_tables(tuple(shape[-2:]), (crop, crop), (out, out))
    return tuple(v.to(dev) if isinstance(v, torch.Tensor) else v for v in t)


def _unpadded_index(w, first, K, n):
    """The input index nearest the middle that is read by some output index and only through non-zero weights."""
    w, first = w.cpu().reshape(-1, K), first.cpu()
    for i in sorted(range(n), key=lambda i: abs(i - n // 2)):
        taps = [(o, i - int(first[o])) for o in range(first.numel()) if 0 <= i - int(first[o]) < K]
        if taps and all(float(w[o, j]) != 0.0 for o, j in taps):
            return i
    raise AssertionError("every input index meets a zero-padded tap")


def _both(x, tabs, out, monkeypatch):
    """(planar result of eqa_crop_resize_aa, channels-last result of eqa_crop_resize_aa_nhwc, its slots)"""
    from equiadapt_amd import ops

    monkeypatch.setenv("EQA_HEAD_FUSED", "0")
    planar = ops.crop_resize_aa(x, tabs, (out, out))
    assert ops.crop_absmax_slots(planar) is None and planar.is_contiguous()
    monkeypatch.setenv("EQA_HEAD_FUSED", "1")
    y = ops.crop_resize_aa(x, tabs, (out, out))
    slots = ops.crop_absmax_slots(y)
    assert slots is not None, "the channels-last form did not run"
    return planar, y, slots


@pytest.mark.parametrize("shape,crop,out", SHAPES)
def test_pixels_are_bit_equal_and_the_slots_hold_the_maximum(dev, monkeypatch, shape, crop, out):
    torch.manual_seed(3)
    x = torch.randn(shape, device=dev)
    tabs = _tables(shape, crop, out, dev)
    planar, y, slots = _both(x, tabs, out, monkeypatch)
    assert y.shape == planar.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert y.contiguous(memory_format=torch.channels_last) is y
    assert torch.equal(y, planar.contiguous(memory_format=torch.channels_last))
    assert torch.equal(y.contiguous(), planar)
    assert slots.max().item() == y.abs().max().item()
    assert bool((slots >= 0).all())


@pytest.mark.parametrize("shape,crop,out", SHAPES)
def test_an_infinity_is_carried_and_a_nan_ignored(dev, monkeypatch, shape, crop, out):
    torch.manual_seed(4)
    tabs = _tables(shape, crop, out, dev)
    x = torch.randn(shape, device=dev)
    # a pixel of the last plane that no zero-padded tap reads (0 * inf would be a NaN, in either kernel)
    yi, xi = _unpadded_index(tabs[2], tabs[3], tabs[4], shape[2]), _unpadded_index(tabs[0], tabs[1], tabs[4], shape[3])
    x[shape[0] - 1, shape[1] - 1, yi, xi] = float("inf")
    planar, y, slots = _both(x, tabs, out, monkeypatch)
    assert torch.isinf(y).any() and not torch.isnan(y).any()
    assert torch.equal(y, planar.contiguous(memory_format=torch.channels_last))
    assert slots.max().item() == y.abs().max().item() == float("inf")
    x[0, 0, shape[2] // 2, shape[3] // 2] = float("nan")
    planar, y, slots = _both(x, tabs, out, monkeypatch)
    assert torch.isnan(y).any()
    assert torch.equal(torch.nan_to_num(y, nan=7.0), torch.nan_to_num(planar.contiguous(memory_format=torch.channels_last), nan=7.0))
    assert not torch.isnan(slots).any()                                               # fmaxf drops the NaN, as eqa_absmax_slots does
    assert slots.max().item() == torch.where(torch.isnan(y), torch.zeros_like(y), y).abs().max().item() == float("inf")


def test_writing_to_the_result_makes_the_slots_stale(dev, monkeypatch):
    from equiadapt_amd import ops

    shape, crop, out = SHAPES[0]
    x = torch.randn(shape, device=dev)
    monkeypatch.setenv("EQA_HEAD_FUSED", "1")
    y = ops.crop_resize_aa(x, _tables(shape, crop, out, dev), (out, out))
    assert ops.crop_absmax_slots(y) is not None
    assert ops.crop_absmax_slots(y.clone()) is None            # another object
    y[0, 0, 0, 0] = 100.0                                     # the same object at another version
    assert ops.crop_absmax_slots(y) is None


def test_refusals(dev):
    from equiadapt_amd import _lib

    lib = _lib.load()
    shape, crop, out = SHAPES[0]
    wx, x0, wy, y0, K, max_rows, xb, xs = _tables(shape, crop, out, dev)
    B, C, H, W = shape
    x = torch.randn(shape, device=dev)
    y = torch.empty((B, out, out, C), device=dev)
    n = lib.eqa_crop_resize_aa_nhwc_slots(B, C, H, W, out, out, K, max_rows, xb, xs)
    assert n > 0 and n % 8 == 0
    slots = torch.empty(n, device=dev)
    ptrs = (x.data_ptr(), y.data_ptr(), wx.data_ptr(), x0.data_ptr(), wy.data_ptr(), y0.data_ptr())

    def call(p=ptrs, C=C, W=W, K=K, xs=xs, out=out, max_rows=max_rows):
        return lib.eqa_crop_resize_aa_nhwc(*p, B, C, H, W, out, out, K, max_rows, xb, xs, slots.data_ptr(), None)

    assert call() == 0
    torch.cuda.synchronize()
    for i in range(6):                                                       # every pointer is needed
        assert call(p=ptrs[:i] + (None,) + ptrs[i + 1:]) == -1
    assert call(K=0) == -1 and call(max_rows=0) == -1 and call(C=0) == -1
    assert lib.eqa_crop_resize_aa_nhwc_slots(B, 0, H, W, out, out, K, max_rows, xb, xs) == -1
    # shapes the caller keeps on eqa_crop_resize_aa: other channel counts, wide filters, rows that are not 16-byte multiples, no
    # column window, a misaligned image, a band wider than the registers hold
    assert call(C=2) == -3 and call(C=4) == -3 and call(K=9) == -3 and call(W=W + 2) == -3 and call(xs=0) == -3
    assert call(p=(x.data_ptr() + 4,) + ptrs[1:]) == -3
    assert lib.eqa_crop_resize_aa_nhwc_slots(B, C, H, W, 64, 200, K, max_rows, xb, xs) == -3
    assert lib.eqa_crop_resize_aa_nhwc_slots(B, 2, H, W, out, out, K, max_rows, xb, xs) == -3
