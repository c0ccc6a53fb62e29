"""Who convolves and who transforms which tile rows in the fused lifting kernel's fp16 form (eqa_lift5_fft48k5_input_f16x2, FORM 2 of
csrc/lift_fft.hip: lf_h2_run deals a sub-phase's 36 tiles to the convolution waves, lf_h2_rows the row passes).  A dealing can go
wrong in three ways: a (tile row, tile column) left to no wave or taken by two, a row pass skipped or run twice, a row pass in front
of the convolution of its rows.  Each leaves whole rows of a tile wrong, i.e. an error of order 1 in every frequency of that tile,
where a rounding change is of order 1e-7.

Reference, bound and helpers are those of test_fused_kernel_on_two_fp16_pieces_matches_fp64_like_the_fp32_form
(tests/test_gpu_lift_fft.py): the whole of V against an fp64 evaluation of relu(conv2d(x, bank) + bias) carried through torch.fft, no
further from it than the fp32 form.  As in tests/test_gpu_lift_patch_fetch.py the images sit at the front of a buffer whose
remaining floats are NaN.

Beside random images every shape is run on images that are CONSTANT ALONG EACH ROW with a different value per row: every lifted row
then differs from its neighbours as a whole, so that a row pass on rows that are not convolved yet (or convolved by the wrong wave)
misses by the size of the data and not by a little."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_lift_fft import _spectra_fp64, _unpack_V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# (nimg, H0, W0, C)
# A: one full tile, one channel group, a single item per launch: no "previous item" for the column waves
# B: three groups; items pipelined across images
# C: 2 x 2 tiles with ragged right and bottom edges: rows and columns past the map in every sub-phase
# D: ragged bottom only
# E: the headline's tile grid
SHAPES = [(1, 52, 52, 16), (2, 52, 52, 48), (1, 57, 53, 32), (1, 60, 96, 16), (2, 96, 96, 32)]


def _images(kind, nimg, H0, W0, g):
    if kind == "random":
        return torch.randn(nimg, H0, W0, 3, generator=g)
    assert kind == "rows"
    return torch.randn(nimg, H0, 1, 3, generator=g).expand(nimg, H0, W0, 3).contiguous()


def _check(dev, kind, nimg, H0, W0, C, relu, with_bias):
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    g = torch.Generator().manual_seed(nimg * 1000 + H0 + C)
    xh = _images(kind, nimg, H0, W0, g)
    if kind == "rows":
        assert (xh[:, :, :1] == xh).all() and (xh[:, 1:, 0] != xh[:, :-1, 0]).all()
    n = xh.numel()
    buf = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=dev)
    buf[:n] = xh.reshape(-1).to(dev)
    x = buf[:n].view(nimg, H0, W0, 3).permute(0, 3, 1, 2)       # (nimg, 3, H0, W0) in channels-last memory; NaN right behind it
    assert x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() == buf.data_ptr()
    bank = (torch.randn(C, 3, 5, 5, generator=g) / 75 ** 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(C, generator=g).to(dev) if with_bias else None
    p_b = bias.data_ptr() if with_bias else None
    M = nimg * fftconv.tiles(H0 - 4) * fftconv.tiles(W0 - 4)
    pitch = lib.eqa_fft48k5_tile_pitch(M)
    st = torch.cuda.current_stream().cuda_stream
    wh, w_scale = fftconv.LiftedInput(x, bank, bias, relu).pieces_f16()
    xb = torch.full((fftconv.DCMAX_SLOTS,), -1.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_absmax_slots(x.data_ptr(), n, xb.data_ptr(), st), "absmax")
    assert xb.max().item() == x.abs().max().item()
    full = torch.full((fftconv.F, pitch, 2 * C), 7.0, dtype=torch.float32, device=dev)
    slots = torch.full((fftconv.DCMAX_SLOTS,), -3.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_lift5_fft48k5_input_f16x2(x.data_ptr(), wh.data_ptr(), w_scale, xb.data_ptr(), fftconv.DCMAX_SLOTS, p_b, int(relu),
                                                 full.data_ptr(), slots.data_ptr() if relu else None, nimg, H0, W0, C, st), "f16x2")
    assert (full[:, M:] == 7.0).all()
    ref = torch.full((fftconv.F, pitch, 2 * C), 7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_lift5_fft48k5_input(x.data_ptr(), bank.data_ptr(), p_b, int(relu), ref.data_ptr(), nimg, H0, W0, C, st), "f32")
    y64 = F.conv2d(x.double(), bank.double(), bias.double() if with_bias else None)
    y64 = torch.relu(y64) if relu else y64
    want = _spectra_fp64(y64)
    scale = want.abs().max().item()
    # the WHOLE of V: every frequency of every tile and channel
    e_h = (_unpack_V(full[:, :M], C) - want).abs().max().item()
    e_f = (_unpack_V(ref[:, :M], C) - want).abs().max().item()
    print(f"conv dealing {kind} {(nimg, H0, W0, C)} relu={relu} bias={with_bias}: "
          f"|f16x2 - fp64| {e_h / scale:.3e}, |f32 - fp64| {e_f / scale:.3e} (of max |V|)")
    assert scale > 0.0
    # the bound of test_fused_kernel_on_two_fp16_pieces_matches_fp64_like_the_fp32_form, as it stands there (a NaN fails both)
    assert e_h <= 3e-6 * scale and e_h <= 1.5 * e_f + 1e-7 * scale, (e_h / scale, e_f / scale)
    if relu:
        assert slots.max().item() == full[48 * 23, :M].max().item() and full[:, :M].abs().max().item() <= slots.max().item()


@pytest.mark.parametrize("nimg,H0,W0,C", SHAPES)
@pytest.mark.parametrize("kind", ["random", "rows"])
def test_every_tile_is_convolved_once_and_every_row_transformed_once_behind_it(dev, kind, nimg, H0, W0, C):
    _check(dev, kind, nimg, H0, W0, C, True, True)


@pytest.mark.parametrize("kind", ["random", "rows"])
def test_dealing_without_relu_and_bias(dev, kind):
    """relu = 0, no bias (and no DC slots): lifted rows of both signs, the ragged 2 x 2 grid."""
    _check(dev, kind, 1, 57, 53, 32, False, False)
