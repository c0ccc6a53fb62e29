"""eqa_fft48k5_cgemm3m_f16x2_k32: the fp16 two-piece contraction ("h3") on v_mfma_f32_16x16x32_f16 -- K-stages of 32 channels, its own
fragment orders for A (LDS) and B (eqa_fft48k5_spectra3m_split_f16_k32), even / odd dealing of a wave's 32 columns over its two column
tiles, 16-byte result stores.  The exact test and the row test also run the form on v_mfma_f32_32x32x16_f16 (eqa_fft48k5_cgemm3m_f16x2)
through its C entry: the two share their argument checks, their launch and the block's walk over its tiles (csrc/cgemm3m_pieces.inc).
F is fixed at 1154, so the shapes are small in M and Cin:

    (5, 64, 128)    one ragged row tile, one column group, two stages, 4-5 tiles per block: tile-to-tile hand-over of the look-ahead
    (129, 96, 128)  a second row tile of one row; three stages (odd: the B ping-pong ends on the other parity)
    (130, 64, 256)  two column groups (ct = 4 cg + wave); the only shape here whose pitch (131) leaves a pad row
    (36, 160, 128)  five stages

Bounds.  Exact test: integer operands, every partial sum below 2^24 and every scaled piece a representable fp16, so fp32 accumulation
commits no rounding and the result must equal the fp64 product bit for bit.  Random operands: the gate of
tests/test_gpu_parity.py::test_fp16_two_piece_gemm_form_is_no_further_from_fp64, unchanged -- the fp32 matrix instruction on the same
inputs is the yardstick (rms no larger, maximum within 5 %)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, 64, 128), (129, 96, 128), (130, 64, 256), (36, 160, 128)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack_b3(Br: torch.Tensor, Bi: torch.Tensor) -> torch.Tensor:
    """A complex (F, Cin, Cout) matrix Br + i Bi -> the flat fp32 operand B3 (F, Cin/16, Cout/32, 3 [Br | Bi | Br + Bi], 2, 64, 4) of
    eqa_fft48k5_cgemm3m, by the index map of include/eqa_hip.h: slot (b, lane = 32 h + i, t) of (f, s, c, part) is channel
    k = 16 s + 8 b + 4 h + t, output channel 32 c + i."""
    Fq, Cin, Cout = Br.shape
    parts = torch.stack([Br, Bi, Br + Bi])                                               # (3, F, Cin, Cout)
    t = parts.reshape(3, Fq, Cin // 16, 2, 2, 4, Cout // 32, 32)                          # (part, f, s, b, h, t, c, i)
    return t.permute(1, 2, 6, 0, 3, 4, 7, 5).contiguous().reshape(-1).float()            # (f, s, c, part, b, h, i, t)


def _fill_v(V: torch.Tensor, Vr: torch.Tensor, Vi: torch.Tensor) -> None:
    """complex (F, M, Cin) Vr + i Vi -> the rows of V: [Re x 16 | Im x 16] per 16 channels."""
    Fq, M, Cin = Vr.shape
    rows = torch.stack([Vr.reshape(Fq, M, Cin // 16, 16), Vi.reshape(Fq, M, Cin // 16, 16)], dim=3)
    V.copy_(rows.reshape(Fq, M, 2 * Cin).float())


def _interleaved(Cr: torch.Tensor, Ci: torch.Tensor) -> torch.Tensor:
    return torch.stack([Cr, Ci], dim=3).reshape(Cr.shape[0], Cr.shape[1], -1)


# the two fp16 forms: (Spectra3M's split, the contraction's entry, the split's entry); every shape has Cin % 32 == 0: both take it
K32 = ("pieces_f16_k32", "eqa_fft48k5_cgemm3m_f16x2_k32", "eqa_fft48k5_spectra3m_split_f16_k32")     # 16x16x32: K-stages of 32
K16 = ("pieces_f16", "eqa_fft48k5_cgemm3m_f16x2", "eqa_fft48k5_spectra3m_split_f16")                 # 32x32x16: K-stages of 16
# the 16x16x32 cases keep the ids they had before the 32x32x16 ones joined them
SHAPES_BY_FORM = ([pytest.param(*s, K32, id="-".join(map(str, s))) for s in SHAPES] +
                  [pytest.param(*s, K16, id="-".join(map(str, s)) + "-32x32x16") for s in SHAPES])


def _h3(lib, form, V, B3, M, bound, out=None):
    """A form's kernel through its C entry on `out` (a whole pitched buffer) or a fresh spectra buffer."""
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    pieces, entry, _ = form
    bk, b_scale = getattr(B3, pieces)()
    Mo = fftconv.spectra_buffer(M, 2 * B3.cout, V.device) if out is None else out
    _lib.check(getattr(lib, entry)(V.data_ptr(), bk.data_ptr(), Mo.data_ptr(), M, B3.cin, B3.cout, bound.data_ptr(), bound.numel(),
                                   b_scale, _stream()), entry)
    return Mo


@pytest.mark.parametrize("M,Cin,Cout,form", SHAPES_BY_FORM)
def test_integer_operands_give_the_fp64_product_exactly(dev, M, Cin, Cout, form):
    """|Re|, |Im| <= 15 on both sides, bound = 16: any error in the fragment order of A or B, in the even / odd dealing of the columns
    or in the store map shows as a wrong number.  The fp32 form on the operand this test packs must give the same product first, so a
    mistake in the packing here shows as one."""
    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    g = torch.Generator().manual_seed(31 * M + Cin + Cout)
    ri = lambda *s: torch.randint(-15, 16, s, generator=g).double().to(dev)
    Vr, Vi, Br, Bi = ri(fftconv.F, M, Cin), ri(fftconv.F, M, Cin), ri(fftconv.F, Cin, Cout), ri(fftconv.F, Cin, Cout)
    want = _interleaved(torch.bmm(Vr, Br) - torch.bmm(Vi, Bi), torch.bmm(Vr, Bi) + torch.bmm(Vi, Br)).float()
    assert want.abs().max().item() < 2 ** 24 and 30 * 30 * Cin < 2 ** 24          # ... and the (re + im).(re + im) product's sums
    B3 = fftconv.Spectra3M(_pack_b3(Br, Bi), Cin, Cout)
    V = fftconv.spectra_buffer(M, 2 * Cin, dev)
    _fill_v(V, Vr, Vi)
    f32 = fftconv.spectra_buffer(M, 2 * Cout, dev)
    _lib.check(lib.eqa_fft48k5_cgemm3m(V.data_ptr(), B3.data.data_ptr(), f32.data_ptr(), M, Cin, Cout, _stream()), "cgemm3m")
    assert torch.equal(f32, want), "the test's own packing of B3 / V"
    bound = torch.full((1,), 16.0, device=dev)
    got = _h3(lib, form, V, B3, M, bound)
    bad = (got != want).nonzero()
    assert torch.equal(got, want), (bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize("M,Cin,Cout", SHAPES)
def test_random_operands_meet_the_h3_gate_and_scale_exactly(dev, M, Cin, Cout, monkeypatch):
    """Two seeds: rms distance to fp64 <= the fp32 matrix instruction's, maximum <= 1.05 x its, also with a bound 16 x too loose;
    contract(8 V, 8 bound) == 8 contract(V, bound) exactly; the bound spread over several slots gives the same bits."""
    from equiadapt_amd.images.canonicalization_networks import fftconv

    assert fftconv.GEMM_PIECES == "auto" and fftconv.gemm_form(Cin, Cout, True) == "h3"
    for seed in (0, 1):
        g = torch.Generator().manual_seed(2000 * seed + M + Cin)
        bank = (torch.randn(Cout, Cin, 5, 5, generator=g) / (5.0 * Cin ** 0.5)).to(dev)
        B, B3 = fftconv.filter_spectra(bank), fftconv.filter_spectra3m(bank)
        V = fftconv.spectra_buffer(M, 2 * Cin, dev)
        V.normal_(generator=torch.Generator(device=dev).manual_seed(seed + 11))
        bound = V.abs().max().reshape(1)
        monkeypatch.setattr(fftconv, "H3_MFMA", "32")
        h32 = fftconv.contract(V, B3, M, bound)
        assert (fftconv.LAST_FORM, fftconv.LAST_H3_MFMA) == ("h3", "32")
        monkeypatch.setattr(fftconv, "H3_MFMA", "16")
        h16 = fftconv.contract(V, B3, M, bound)
        assert (fftconv.LAST_FORM, fftconv.LAST_H3_MFMA) == ("h3", "16")
        loose = fftconv.contract(V, B3, M, bound * 16.0)
        V8 = fftconv.spectra_buffer(M, 2 * Cin, dev)
        V8.copy_(V * 8.0)
        assert torch.equal(fftconv.contract(V8, B3, M, bound * 8.0), h16 * 8.0)
        slots = torch.zeros(256, device=dev)
        slots[17] = bound[0]
        slots[200] = bound[0] * 0.5
        assert torch.equal(fftconv.contract(V, B3, M, slots), h16)
        monkeypatch.setattr(fftconv, "GEMM_PIECES", "f32")
        f32 = fftconv.contract(V, B3, M)
        assert fftconv.LAST_FORM == "f32"
        monkeypatch.setattr(fftconv, "GEMM_PIECES", "auto")
        want = torch.bmm(V.double(), B.double())
        err = {}
        for name, got in (("h16", h16), ("h32", h32), ("f32", f32), ("loose", loose)):
            d = got.double() - want
            err[name] = (d.abs().max().item(), d.pow(2).mean().sqrt().item())
        print(f"h3 k32 gate {(M, Cin, Cout)} seed {seed}: 16x16x32 max {err['h16'][0]:.3e} rms {err['h16'][1]:.3e} | 32x32x16 max "
              f"{err['h32'][0]:.3e} rms {err['h32'][1]:.3e} | f32 max {err['f32'][0]:.3e} rms {err['f32'][1]:.3e} | bound x 16: max "
              f"{err['loose'][0]:.3e} rms {err['loose'][1]:.3e}")
        for name in ("h16", "h32", "loose"):
            assert err[name][1] <= err["f32"][1], (M, Cin, Cout, seed, name, err)
            assert err[name][0] <= 1.05 * err["f32"][0], (M, Cin, Cout, seed, name, err)


@pytest.mark.parametrize("M,Cin,Cout,form", SHAPES_BY_FORM)
def test_rows_beyond_m_are_neither_written_nor_read_into_rows_below(dev, M, Cin, Cout, form):
    """Mo's pitched buffer and a guard behind it keep a sentinel outside rows < M; NaN in the pad rows of V changes no row < M."""
    import math

    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    g = torch.Generator().manual_seed(M + Cout)
    bank = (torch.randn(Cout, Cin, 5, 5, generator=g) / (5.0 * Cin ** 0.5)).to(dev)
    B3 = fftconv.filter_spectra3m(bank)
    pitch = lib.eqa_fft48k5_tile_pitch(M)
    Vfull = torch.randn(fftconv.F, pitch, 2 * Cin, generator=g).to(dev)
    bound = Vfull[:, :M].abs().max().reshape(1)
    n, guard = fftconv.F * pitch * 2 * Cout, 128 * 2 * Cout
    flat = torch.full((n + guard,), 7.0, dtype=torch.float32, device=dev)
    full = flat[:n].view(fftconv.F, pitch, 2 * Cout)
    _h3(lib, form, Vfull, B3, M, bound, out=full)
    assert (full[:, M:] == 7.0).all() and (flat[n:] == 7.0).all()
    assert not (full[:, :M] == 7.0).any()
    Vnan = Vfull.clone()
    Vnan[:, M:] = math.nan
    again = torch.full_like(full, 7.0)
    _h3(lib, form, Vnan, B3, M, bound, out=again)
    assert torch.equal(again, full)
    # the argument checks of the form's two entries
    pieces, entry, split_entry = form
    bk, b_scale = getattr(B3, pieces)()
    contract, split = getattr(lib, entry), getattr(lib, split_entry)
    args = (Vfull.data_ptr(), bk.data_ptr(), full.data_ptr())
    assert contract(*args, M, Cin, Cout, None, 1, b_scale, _stream()) == -1
    assert contract(*args, M, Cin, Cout, bound.data_ptr(), 0, b_scale, _stream()) == -1
    assert contract(*args, M, Cin, Cout, bound.data_ptr(), 1, 0.0, _stream()) == -1
    assert contract(*args, M, Cin, 64, bound.data_ptr(), 1, b_scale, _stream()) == -3
    assert contract(*args, 0, Cin, Cout, bound.data_ptr(), 1, b_scale, _stream()) == 0
    assert split(B3.data.data_ptr(), bk.data_ptr(), Cin, Cout, 3.0, _stream()) == -1
    assert split(B3.data.data_ptr(), bk.data_ptr(), Cin, 64, b_scale, _stream()) == -3


def test_k32_pieces_are_built_once_per_weight_version(dev, monkeypatch):
    """`Spectra3M.pieces_f16_k32()` is split on first use and kept; spectra derived from a parameter through `DerivedCache` (how the
    networks hold them) are rebuilt, and split again, once the parameter's storage has been swapped or written in place."""
    from equiadapt_amd import _lib
    from equiadapt_amd.common.derived import DerivedCache
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    M, Cin, Cout = 5, 64, 128
    calls = []
    split = lib.eqa_fft48k5_spectra3m_split_f16_k32
    monkeypatch.setattr(lib, "eqa_fft48k5_spectra3m_split_f16_k32", lambda *a: (calls.append(1), split(*a))[1])
    monkeypatch.setattr(fftconv, "H3_MFMA", "16")
    g = torch.Generator().manual_seed(5)
    w = torch.nn.Parameter((torch.randn(Cout, Cin, 5, 5, generator=g) / (5.0 * Cin ** 0.5)).to(dev))
    V = fftconv.spectra_buffer(M, 2 * Cin, dev)
    V.normal_(generator=torch.Generator(device=dev).manual_seed(3))
    bound = V.abs().max().reshape(1)
    cache = DerivedCache()

    def run():
        cache.get("bank", [w], lambda: w.detach())
        B3 = cache.derived("bank", "fft", lambda: fftconv.spectra_for(w.detach()))
        return fftconv.contract(V, B3, M, bound).clone(), B3

    first, B3a = run()
    second, B3b = run()
    assert B3b is B3a and len(calls) == 1 and torch.equal(first, second)
    assert B3a.pieces_f16_k32()[0] is B3a.pieces_f16_k32()[0] and len(calls) == 1
    version = w._version
    w.data = w.data.clone() * 1.5                                  # the storage swapped under the same tensor, same version
    assert w._version == version
    third, B3c = run()
    assert B3c is not B3a and len(calls) == 2
    assert torch.equal(third, fftconv.contract(V, fftconv.spectra_for(w.detach()), M, bound)) and not torch.equal(third, first)
    with torch.no_grad():
        w.mul_(2.0)                                                # written in place
    fourth, B3d = run()
    assert B3d is not B3c and torch.equal(fourth, fftconv.contract(V, fftconv.spectra_for(w.detach()), M, bound))
    assert not torch.equal(fourth, third)
