"""FORM 2 of csrc/lift_fft.hip (eqa_lift5_fft48k5_input_f16x2) with its convolution on four waves, one per SIMD: each wave takes
nine of a sub-phase's 36 tiles in column-major order, two of them cross from one tile column to the next.  The shapes below stress
that split and the re-placed row transforms: a single item, item counts that do not fill or divide the 256 blocks, 16 / 32 / 256
channels, non-square maps and last tile rows / columns that end inside a wave's share.  Every case is held to an fp64 evaluation
of relu(conv2d(x, bank) + bias) carried through the tiles' FFT, at the rule of test_gpu_lift_fft.py's fp16 test, and to the fp32
form (eqa_lift5_fft48k5_input) on the same operands."""
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
    tiles = torch.stack([yp[:, :, 44 * ty:44 * ty + 48, 44 * tx:44 * tx + 48] for ty in range(TY) for tx in range(TX)], dim=1)
    spec = torch.fft.rfft2(tiles)
    ky, kx = fftconv.freq_index()
    return spec[..., ky.to(y.device), kx.to(y.device)].reshape(nimg * TY * TX, C, -1).permute(2, 0, 1)


def _unpack_V(V: torch.Tensor, C: int):
    Fq, M, _ = V.shape
    v = V.double().reshape(Fq, M, C // 16, 2, 16)
    return torch.complex(v[:, :, :, 0], v[:, :, :, 1]).reshape(Fq, M, C)


# (nimg, H0, W0, C): the lifted map is (H0 - 4) x (W0 - 4), its last tile keeps rows / columns 44 (T - 1) .. H1 - 1
CASES = [
    (1, 52, 52, 16),      # one item: one block
    (1, 52, 52, 256),     # 16 items, one per group
    (3, 96, 96, 32),      # 24 items
    (7, 96, 96, 256),     # 448 items on 256 blocks: some blocks take two, some one
    (2, 60, 101, 32),     # non-square; last tile: 12 rows (one sub-phase), 9 columns
    (3, 101, 60, 16),     # the transpose: last tile 9 rows (wave 8's share of a sub-phase), 12 columns
    (2, 73, 117, 16),     # last tile rows end at 25 (inside sub-phase 2, in the middle of a crossing wave's share), 25 columns
    (1, 143, 56, 256),    # last tile: 7 rows (inside wave 8's share of sub-phase 0), 8 columns (inside tile column 0)
]


@pytest.mark.parametrize("nimg,H0,W0,C", CASES)
@pytest.mark.parametrize("relu,with_bias", [(True, True), (False, False)])
def test_four_simd_convolution_matches_fp64_and_the_fp32_form(dev, nimg, H0, W0, C, relu, with_bias):
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    g = torch.Generator().manual_seed(nimg * 7919 + H0 * 31 + W0 + C)
    x = torch.randn(nimg, 3, H0, W0, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    bank = (torch.randn(C, 3, 5, 5, generator=g) / 75 ** 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(C, generator=g).to(dev) if with_bias else None
    p_b = bias.data_ptr() if with_bias else None
    M = nimg * fftconv.tiles(H0 - 4) * fftconv.tiles(W0 - 4)
    pitch = lib.eqa_fft48k5_tile_pitch(M)
    st = torch.cuda.current_stream().cuda_stream
    wh, w_scale = fftconv.LiftedInput(x, bank, bias, relu).pieces_f16()
    xb = torch.empty(fftconv.DCMAX_SLOTS, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_absmax_slots(x.data_ptr(), x.numel(), xb.data_ptr(), st), "absmax")
    got = torch.full((fftconv.F, pitch, 2 * C), 7.0, dtype=torch.float32, device=dev)
    slots = torch.full((fftconv.DCMAX_SLOTS,), -3.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_lift5_fft48k5_input_f16x2(x.data_ptr(), wh.data_ptr(), w_scale, xb.data_ptr(), fftconv.DCMAX_SLOTS, p_b, int(relu),
                                                 got.data_ptr(), slots.data_ptr() if relu else None, nimg, H0, W0, C, st), "f16x2")
    ref = torch.full((fftconv.F, pitch, 2 * C), 7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_lift5_fft48k5_input(x.data_ptr(), bank.data_ptr(), p_b, int(relu), ref.data_ptr(), nimg, H0, W0, C, st), "f32")
    torch.cuda.synchronize()
    assert (got[:, M:] == 7.0).all()
    y64 = F.conv2d(x.double(), bank.double(), bias.double() if with_bias else None)
    want = _spectra_fp64(torch.relu(y64) if relu else y64)
    scale = want.abs().max().item()
    e_h = (_unpack_V(got[:, :M], C) - want).abs().max().item()
    e_f = (_unpack_V(ref[:, :M], C) - want).abs().max().item()
    e_hf = (_unpack_V(got[:, :M], C) - _unpack_V(ref[:, :M], C)).abs().max().item()
    print(f"f16x2 {(nimg, H0, W0, C)} relu={relu}: |f16x2 - fp64| {e_h / scale:.3e}, |f32 - fp64| {e_f / scale:.3e}, "
          f"|f16x2 - f32| {e_hf / scale:.3e} (of max |V|)")
    assert e_h <= 3e-6 * scale and e_h <= 1.5 * e_f + 1e-7 * scale, (e_h / scale, e_f / scale)
    if relu:
        assert slots.max().item() == got[48 * 23, :M].max().item() and got[:, :M].abs().max().item() <= slots.max().item()


def test_four_simd_convolution_is_deterministic(dev):
    """Two launches on the same operands give the same bits (every output pixel keeps one order of products and sums)."""
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    nimg, H0, W0, C = 5, 96, 96, 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(nimg, 3, H0, W0, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    bank = (torch.randn(C, 3, 5, 5, generator=g) / 75 ** 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(C, generator=g).to(dev)
    M = nimg * fftconv.tiles(H0 - 4) * fftconv.tiles(W0 - 4)
    pitch = lib.eqa_fft48k5_tile_pitch(M)
    st = torch.cuda.current_stream().cuda_stream
    wh, w_scale = fftconv.LiftedInput(x, bank, bias, True).pieces_f16()
    xb = torch.empty(fftconv.DCMAX_SLOTS, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_absmax_slots(x.data_ptr(), x.numel(), xb.data_ptr(), st), "absmax")
    outs = []
    for _ in range(2):
        V = torch.zeros((fftconv.F, pitch, 2 * C), dtype=torch.float32, device=dev)
        _lib.check(lib.eqa_lift5_fft48k5_input_f16x2(x.data_ptr(), wh.data_ptr(), w_scale, xb.data_ptr(), fftconv.DCMAX_SLOTS, bias.data_ptr(), 1,
                                                     V.data_ptr(), None, nimg, H0, W0, C, st), "f16x2")
        outs.append(V)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
