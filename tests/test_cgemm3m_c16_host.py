"""Host side of the 16-multiple channel contractions (csrc/cgemm3m_c16.hip): the shape predicates, the size of the packed filter
operand, what the entry points refuse before any launch, and `Spectra3MC16.unpack` against the layout include/eqa_hip.h documents.
No GPU: every call here returns before it would launch (fake, never dereferenced pointers)."""
import pytest
import torch

from equiadapt_amd import _lib
from equiadapt_amd.images.canonicalization_networks import fftconv

OK, INVALID, UNSUPPORTED = 0, -1, -3
P = 0x7F0000001000        # a 16-byte aligned address that is never dereferenced


def test_predicates():
    lib = _lib.load()
    for fn in (lib.eqa_fft48_cgemm3m_c16_supported, lib.eqa_fft48_wgrad3m_c16_supported):
        for cin, cout in [(16, 16), (144, 144), (48, 80), (288, 288)]:
            assert fn(cin, cout) == 1, (cin, cout)
        for cin, cout in [(8, 16), (144, 150), (0, 16), (16, 0), (-16, 16), (16, 24)]:
            assert fn(cin, cout) == 0, (cin, cout)


def test_existing_predicate_answers_as_before():
    lib = _lib.load()
    for (cin, cout), want in {(48, 64): 0, (64, 32): 0, (144, 144): 0, (16, 64): 0, (32, 64): 1, (64, 64): 1, (256, 256): 1, (0, 64): 0}.items():
        assert lib.eqa_fft48k5_cgemm3m_supported(cin, cout) == want, (cin, cout)
    assert lib.eqa_fft48k5_spectra3m_floats(256, 256) == 1154 * 256 * 256 * 3 and lib.eqa_fft48k5_spectra3m_floats(144, 144) == 0
    assert lib.eqa_fft48k5_wgrad3m_supported(144, 144) == 0 and lib.eqa_fft48k5_wgrad3m_supported(64, 128) == 1


def test_operand_size():
    lib = _lib.load()
    assert lib.eqa_fft48k5_frequencies() == 1154
    assert lib.eqa_fft48_spectra3m_c16_floats(144, 144) == 1154 * 144 * 160 * 3
    assert lib.eqa_fft48_spectra3m_c16_floats(16, 16) == 1154 * 16 * 32 * 3
    assert lib.eqa_fft48_spectra3m_c16_floats(48, 80) == 1154 * 48 * 96 * 3
    assert lib.eqa_fft48_spectra3m_c16_floats(288, 288) == 1154 * 288 * 288 * 3
    assert lib.eqa_fft48_spectra3m_c16_floats(8, 16) == 0 and lib.eqa_fft48_spectra3m_c16_floats(144, 150) == 0


@pytest.mark.parametrize("name", ["eqa_fft48_cgemm3m_c16", "eqa_fft48_wgrad3m_c16"])
def test_contractions_refuse_before_launch(name):
    fn = getattr(_lib.load(), name)
    for bad in range(3):
        ptrs = [P, P + 0x100000, P + 0x200000]
        ptrs[bad] = None
        assert fn(*ptrs, 8, 144, 144, None) == INVALID
        ptrs[bad] = P + 8 + 0x100000 * bad                  # 8-byte aligned only
        assert fn(*ptrs, 8, 144, 144, None) == UNSUPPORTED
    assert fn(P, P, P, -1, 144, 144, None) == INVALID
    assert fn(P, P, P, 8, 0, 144, None) == INVALID and fn(P, P, P, 8, 144, -16, None) == INVALID
    assert fn(P, P, P, 8, 144, 150, None) == UNSUPPORTED and fn(P, P, P, 8, 8, 16, None) == UNSUPPORTED
    # ranges a 32-bit buffer descriptor cannot hold: too many tiles, one frequency of V / Mo beyond 2^31 bytes
    assert fn(P, P, P, 0x400000, 16, 16, None) == UNSUPPORTED
    assert fn(P, P, P, 1 << 20, 4096, 16, None) == UNSUPPORTED and fn(P, P, P, 1 << 20, 16, 4096, None) == UNSUPPORTED
    # nothing to do
    assert fn(P, P, P, 0, 144, 144, None) == OK
    assert fn(P + 8, P, P, 0, 144, 144, None) == OK and fn(None, P, P, 0, 144, 144, None) == INVALID


@pytest.mark.parametrize("k5", [True, False])
def test_filter_operand_refuses_before_launch(k5):
    lib = _lib.load()
    fn = (lambda b, o, co, ci: lib.eqa_fft48k5_filter_spectra3m_c16(b, o, co, ci, 1, None)) if k5 else \
         (lambda b, o, co, ci: lib.eqa_fft48_filter_spectra3m_c16(b, o, co, ci, 7, 1, None))
    assert fn(None, P, 144, 144) == INVALID and fn(P, None, 144, 144) == INVALID and fn(P, P, 0, 144) == INVALID
    assert fn(P, P + 8, 144, 144) == UNSUPPORTED and fn(P, P, 150, 144) == UNSUPPORTED and fn(P, P, 144, 8) == UNSUPPORTED


@pytest.mark.parametrize("cin,cout", [(16, 16), (48, 80), (32, 144)])
def test_unpack_follows_the_documented_layout(cin, cout):
    """B3 (F, Cin/16, ceil(Cout/32), 3, 2, 64 [lane = 32 h + j], 4 [t]): input channel 16 s + 8 b + 4 h + t, output channel 32 c + j."""
    nct = (cout + 31) // 32
    n = fftconv.F * cin * nct * 32 * 3
    data = torch.arange(n, dtype=torch.float64).remainder(1 << 24).float()         # every element recognisable
    sp = fftconv.Spectra3MC16(data, cin, cout)
    parts = sp.unpack(pad=True)
    assert all(p.shape == (fftconv.F, cin, nct * 32) for p in parts)
    assert all(p.shape == (fftconv.F, cin, cout) for p in sp.unpack())
    g = torch.Generator().manual_seed(cin + cout)
    for _ in range(200):
        f, k, col, part = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (fftconv.F, cin, nct * 32, 3))
        s, b, h, t = k // 16, (k % 16) // 8, (k % 8) // 4, k % 4
        c, j = col // 32, col % 32
        flat = (((((f * (cin // 16) + s) * nct + c) * 3 + part) * 2 + b) * 64 + 32 * h + j) * 4 + t
        assert parts[part][f, k, col] == data[flat]


def test_routing_predicate_and_knob(monkeypatch):
    """`gemm3m_c16_supported`: only what the existing kernel leaves to the library, only under GEMM == "3m", and not with the knob off."""
    assert fftconv.gemm3m_c16_supported(144, 144) and fftconv.gemm3m_c16_supported(48, 80) and fftconv.gemm3m_c16_supported(64, 32)
    assert not fftconv.gemm3m_c16_supported(256, 256) and not fftconv.gemm3m_c16_supported(144, 150)
    assert fftconv.gemm3m_supported(256, 256) and not fftconv.gemm3m_supported(144, 144)
    monkeypatch.setattr(fftconv, "GEMM_C16", False)
    assert not fftconv.gemm3m_c16_supported(144, 144) and fftconv.gemm3m_supported(256, 256)
    monkeypatch.setattr(fftconv, "GEMM_C16", True)
    monkeypatch.setattr(fftconv, "GEMM", "lib")
    assert not fftconv.gemm3m_c16_supported(144, 144) and not fftconv.gemm3m_supported(256, 256)
