"""Sub-phase 0 of the fused lifting kernel's fp16 form (eqa_lift5_fft48k5_input_f16x2, FORM 2 of csrc/lift_fft.hip): wave 0's packed
columns and the sub-phase's convolution dealing.

Wave 0 transforms the columns kx = 0 and kx = 24 of a tile as ONE complex column (kx = 0 in the real part, kx = 24 in the imaginary
part) and separates them afterwards: C0[ky] and C24[ky] from Z[ky] and Z[48 - ky].  With EQA_LF_H2_PACKED = 1 that happens when a
frequency group is stored, in three different sub-phases, from registers that other code (a row pass, the next group's store) shares.
What can go wrong:

  * a partner Z[48 - ky] that is no longer in its register when group g leaves (stored and transposed away, or overwritten by a row
    pass): C0 and C24 of whole frequency groups wrong by the size of the data;
  * C0 and C24 swapped, conjugated wrongly or written to each other's line;
  * the DC slot taken from Z[0] instead of C0[0];
  * a tile of sub-phase 0 convolved by no wave or by two (lf_h2_run takes the sub-phase: a dealing may treat sub-phase 0, in which
    the column waves transform, differently from the others).

The images that single these out: CONSTANT ALONG x without bias and relu, so that the whole lifted map of a full-width tile lies in
the kx = 0 column (C24 must vanish, C0 carries everything), and ALTERNATING IN SIGN ALONG x, which puts all of it into kx = 24 (C0 must
vanish).  Both take a different value per row, so a wrong row dealing shows too.

Shapes: one item per block; 272 items on 256 blocks, so that a column wave holds a pending item (whose packed columns it separates
group by group) while the next one is convolved and row-transformed; ragged right and bottom edges.  Reference and bound are those of
tests/test_gpu_lift_conv_dealing.py (the whole of V against the fp64 evaluation, 3e-6 of the largest bin and no further than 1.5 x
the fp32 form), NaN behind the input buffer."""
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
SHAPES = [(2, 96, 96, 32), (17, 52, 52, 256), (5, 57, 53, 256)]
# (images, relu, bias)
INPUTS = [("random", False, False), ("const_x", False, False), ("alt_x", False, False), ("random", True, True)]


def _images(kind, nimg, H0, W0, g):
    if kind == "random":
        return torch.randn(nimg, H0, W0, 3, generator=g)
    rows = torch.randn(nimg, H0, 1, 3, generator=g)
    if kind == "const_x":
        return rows.expand(nimg, H0, W0, 3).contiguous()
    assert kind == "alt_x"
    sign = torch.tensor([1.0, -1.0]).repeat((W0 + 1) // 2)[:W0].view(1, 1, W0, 1)
    return (rows * sign).contiguous()


def test_shapes_are_what_they_are_chosen_for():
    """One item per block, more items than blocks, ragged edges; every shape has a tile the map fills from left to right."""
    from equiadapt_amd.images.canonicalization_networks import fftconv

    for (nimg, H0, W0, C), two in zip(SHAPES, (False, True, True)):
        ngrp = C // 16
        nwork = nimg * fftconv.tiles(H0 - 4) * fftconv.tiles(W0 - 4) * ngrp
        nblk = min((256 // ngrp) * ngrp, nwork)
        assert (nwork > nblk) == two and nwork <= 2 * nblk, (nimg, H0, W0, C, nwork, nblk)
        assert W0 - 4 >= 48


@pytest.mark.parametrize("nimg,H0,W0,C", SHAPES)
@pytest.mark.parametrize("kind,relu,with_bias", INPUTS, ids=["random", "const_x", "alt_x", "random_relu_bias"])
def test_packed_columns_and_sub_phase_0(dev, kind, relu, with_bias, nimg, H0, W0, C):
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    g = torch.Generator().manual_seed(nimg * 1000 + H0 + C)
    xh = _images(kind, nimg, H0, W0, g)
    n = xh.numel()
    buf = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=dev)
    buf[:n] = xh.reshape(-1).to(dev)
    x = buf[:n].view(nimg, H0, W0, 3).permute(0, 3, 1, 2)       # (nimg, 3, H0, W0) in channels-last memory; NaN right behind it
    assert x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() == buf.data_ptr()
    bank = (torch.randn(C, 3, 5, 5, generator=g) / 75 ** 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(C, generator=g).to(dev) if with_bias else None
    p_b = bias.data_ptr() if with_bias else None
    TY, TX = fftconv.tiles(H0 - 4), fftconv.tiles(W0 - 4)
    M = nimg * TY * TX
    pitch = lib.eqa_fft48k5_tile_pitch(M)
    st = torch.cuda.current_stream().cuda_stream
    wh, w_scale = fftconv.LiftedInput(x, bank, bias, relu).pieces_f16()
    xb = torch.full((fftconv.DCMAX_SLOTS,), -1.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_absmax_slots(x.data_ptr(), n, xb.data_ptr(), st), "absmax")
    full = torch.full((fftconv.F, pitch, 2 * C), 7.0, dtype=torch.float32, device=dev)
    slots = torch.full((fftconv.DCMAX_SLOTS,), -3.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_lift5_fft48k5_input_f16x2(x.data_ptr(), wh.data_ptr(), w_scale, xb.data_ptr(), fftconv.DCMAX_SLOTS, p_b, int(relu),
                                                 full.data_ptr(), slots.data_ptr() if relu else None, nimg, H0, W0, C, st), "f16x2")
    assert (full[:, M:] == 7.0).all()
    ref = torch.full((fftconv.F, pitch, 2 * C), 7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.eqa_lift5_fft48k5_input(x.data_ptr(), bank.data_ptr(), p_b, int(relu), ref.data_ptr(), nimg, H0, W0, C, st), "f32")
    y64 = F.conv2d(x.double(), bank.double(), bias.double() if with_bias else None)
    y64 = torch.relu(y64) if relu else y64
    want = _spectra_fp64(y64)                                    # (F, M, C)
    got = _unpack_V(full[:, :M], C)
    scale = want.abs().max().item()
    e_h = (got - want).abs().max().item()
    e_f = (_unpack_V(ref[:, :M], C) - want).abs().max().item()
    print(f"sub-phase 0 {kind} {(nimg, H0, W0, C)} relu={relu} bias={with_bias}: "
          f"|f16x2 - fp64| {e_h / scale:.3e}, |f32 - fp64| {e_f / scale:.3e} (of max |V|)")
    assert scale > 0.0
    # the bound of tests/test_gpu_lift_conv_dealing.py, as it stands there (a NaN fails both)
    assert e_h <= 3e-6 * scale and e_h <= 1.5 * e_f + 1e-7 * scale, (e_h / scale, e_f / scale)
    ky, kx = fftconv.freq_index()
    dc = int(((ky == 0) & (kx == 0)).nonzero().item())
    assert dc == 48 * 23
    if relu:
        # the DC slots: the largest DC bin the kernel stored, which bounds every entry of V -- and is the evaluation's largest DC bin
        assert slots.max().item() == full[dc, :M].max().item() and full[:, :M].abs().max().item() <= slots.max().item()
        dc_want = want[dc].real.max().item()
        print(f"  largest DC slot {slots.max().item():.6g}, fp64 {dc_want:.6g}")
        assert abs(slots.max().item() - dc_want) <= 3e-6 * scale
    if kind in ("const_x", "alt_x"):
        # tiles the map fills from left to right: there every lifted row is constant (alternating) over all 48 columns
        full_w = torch.tensor([44 * tx + 48 <= W0 - 4 for _ in range(nimg) for _ in range(TY) for tx in range(TX)], device=dev)
        assert full_w.any()
        lives, vanishes = (0, 24) if kind == "const_x" else (24, 0)
        f_live, f_zero = (kx == lives).nonzero().flatten().to(dev), (kx == vanishes).nonzero().flatten().to(dev)
        assert f_live.numel() == 25 and f_zero.numel() == 25
        other = torch.ones(fftconv.F, dtype=torch.bool, device=dev)
        other[f_live] = False
        z_want = want[f_zero][:, full_w].abs().max().item()
        z_got = got[f_zero][:, full_w].abs().max().item()
        rest = got[other][:, full_w].abs().max().item()
        print(f"  column kx = {vanishes} of the full-width tiles: {z_got / scale:.3e} (fp64 {z_want / scale:.3e}), every column but kx = {lives}: "
              f"{rest / scale:.3e} (of max |V|)")
        assert z_want <= 1e-12 * scale and want[f_live][:, full_w].abs().max().item() > 0.0
        assert z_got <= 3e-6 * scale and rest <= 3e-6 * scale, (z_got / scale, rest / scale)
