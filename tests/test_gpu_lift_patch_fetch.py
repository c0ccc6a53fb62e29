"""The patch fetch of the fused lifting kernel's fp16 form (eqa_lift5_fft48k5_input_f16x2, FORM 2 of csrc/lift_fft.hip): a pixel's
three channels arrive in ONE load.  What such a fetch can get wrong -- a dropped or misplaced channel, a pixel beyond the image that
is not zero, a read past the end of the images -- shows as an error of order 1 against an fp64 evaluation of
relu(conv2d(x, bank) + bias) carried through torch.fft; a rounding change is of order 1e-7.  Tolerances, reference and helpers are
those of test_fused_kernel_on_two_fp16_pieces_matches_fp64_like_the_fp32_form (tests/test_gpu_lift_fft.py).

The images sit at the FRONT of a buffer whose remaining floats are NaN (the allocator rounds a tensor's size up, so "exactly its
size" is not available): the last pixel of the last patch row ends the images, and whatever a fetch reads beyond them poisons V."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _spectra_fp64(y: torch.Tensor):
    """(nimg, C, H1, W1) fp64 map -> the (F, M, C) complex spectra of its 48 x 48 tiles at stride 44 (zero beyond the map)."""
    from equiadapt_amd.images.canonicalization_networks import fftconv

    nimg, C, H1, W1 = y.shape
    TY, TX = fftconv.tiles(H1), fftconv.tiles(W1)
    yp = torch.zeros(nimg, C, 44 * (TY - 1) + 48, 44 * (TX - 1) + 48, dtype=y.dtype, device=y.device)
    yp[:, :, :H1, :W1] = y
    tiles = torch.stack([yp[:, :, 44 * ty:44 * ty + 48, 44 * tx:44 * tx + 48] for ty in range(TY) for tx in range(TX)], dim=1)   # (nimg, T, C, 48, 48)
    spec = torch.fft.rfft2(tiles)                                                                     # (nimg, T, C, 48, 25)
    ky, kx = fftconv.freq_index()
    return spec[..., ky.to(y.device), kx.to(y.device)].reshape(nimg * TY * TX, C, -1).permute(2, 0, 1)  # (F, M, C)


def _unpack_V(V: torch.Tensor, C: int):
    """(F, M, 2C) fp32 rows in [Re x 16 | Im x 16] groups -> (F, M, C) complex128."""
    Fq, M, _ = V.shape
    v = V.double().reshape(Fq, M, C // 16, 2, 16)
    return torch.complex(v[:, :, :, 0], v[:, :, :, 1]).reshape(Fq, M, C)


def _check(dev, nimg, H0, W0, C, relu, with_bias, only_channel=None):
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    g = torch.Generator().manual_seed(nimg * 1000 + H0 + C)
    xh = torch.randn(nimg, H0, W0, 3, generator=g)
    if only_channel is not None:
        keep = torch.zeros(3)
        keep[only_channel] = 1.0
        xh = xh * keep
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
    e_h = (_unpack_V(full[:, :M], C) - want).abs().max().item()
    e_f = (_unpack_V(ref[:, :M], C) - want).abs().max().item()
    print(f"patch fetch {(nimg, H0, W0, C)} relu={relu} bias={with_bias} only_channel={only_channel}: "
          f"|f16x2 - fp64| {e_h / scale:.3e}, |f32 - fp64| {e_f / scale:.3e} (of max |V|)")
    assert scale > 0.0
    assert e_h <= 3e-6 * scale and e_h <= 1.5 * e_f + 1e-7 * scale, (e_h / scale, e_f / scale)   # (a NaN fails both)


# A: one tile, one channel group; the last pixel of the last patch row ends the images
# B: rows of 684 bytes (not 16-byte aligned); a second tile row and column whose patches lie almost wholly outside the image
# C: the headline geometry (a tile at gx0 = 44: byte offset 528), the image stride, two channel groups
# D: three tile rows, patch rows beyond H0, odd W0
SHAPES = [(1, 52, 52, 16), (1, 53, 57, 16), (2, 96, 96, 32), (1, 100, 97, 16)]


@pytest.mark.parametrize("nimg,H0,W0,C", SHAPES)
@pytest.mark.parametrize("relu,with_bias", [(True, True), (False, False)])
def test_patch_fetch_delivers_every_pixel_and_zeros_beyond_the_image(dev, nimg, H0, W0, C, relu, with_bias):
    _check(dev, nimg, H0, W0, C, relu, with_bias)


@pytest.mark.parametrize("channel", [1, 2])
@pytest.mark.parametrize("relu,with_bias", [(True, True), (False, False)])
def test_patch_fetch_delivers_each_channel(dev, channel, relu, with_bias):
    """E: shape A with every channel but one zero: a fetch that delivers channel 0 alone (or a channel in another's place) leaves
    spectra that are not the fp64 ones."""
    _check(dev, 1, 52, 52, 16, relu, with_bias, only_channel=channel)
