"""5x5 stride-1 convolutions as an overlap-save FFT convolution on 48x48 tiles: the regular -> regular layers of the
canonicalization network (reference: equiadapt/images/canonicalization_networks/escnn_networks.py:67-91) in inference
(`conv5x5`) and in training (`conv5x5` with ``keep_V``, `grad_spectra`, `filter_grad`, `input_grad`; used by
`winograd.Conv5x5Function`).

48x48 real FFT tiles produce 44x44 outputs each; per frequency the channel contraction is a complex matrix product that the
GEMM library runs as a real one (see include/eqa_hip.h, eqa_fft48k5_*).  Where the tiles fit the output (88 = 2 x 44 at the
headline shape) this needs 2.5 real multiplies per output against 4 for Winograd F(4x4,5x5), and spectra of 1.24x the
activation size against 4x.  fp32 throughout."""
import ctypes
import math
import os
from typing import Optional

import torch

from equiadapt_amd import _lib, ops
from equiadapt_amd.ops import _timed

N, NH, OUT = 48, 25, 44
F = N * (NH - 2) + 2 * NH     # 1154 stored frequencies: the conjugate-redundant half of the kx = 0 / 24 columns is dropped
ENABLED = os.environ.get("EQA_CONV5_FFT", "1") != "0"
# The filter spectra (1154 x 2Cin x 2Cout floats: 1.21 GB at 256 channels) are streamed once per call, the Winograd filters are
# 17 MB: below ~32 tiles (8 images of 92 x 92) the Winograd path is faster (measured: B=4 0.29 vs 0.37 ms, B=8 0.48 vs 0.46 ms).
MIN_TILES = int(os.environ.get("EQA_FFT_MIN_TILES", "32"))
TRAIN_FORWARD = os.environ.get("EQA_FFT_TRAIN", "1") != "0"     # forward pass of winograd.Conv5x5Function through this path
# The per-frequency channel contraction: "3m" = the hand-written complex GEMM on the fp32 MFMA in the 3-multiplication form
# (eqa_fft48k5_cgemm3m; channel counts it takes: Cin % 32 == 0, Cout % 64 == 0; other multiples of 16: eqa_fft48_cgemm3m_c16, see
# GEMM_C16 below), "lib" = the library's real batched GEMM.
GEMM = os.environ.get("EQA_FFT_GEMM", "3m")
# How the hand-written GEMM multiplies: "f32" = the fp32 matrix instruction; "9" / "6" = every fp32 operand split exactly into three
# bf16 pieces and that many piece products on the bf16 matrix cores (eqa_fft48k5_cgemm3m_bf16x3: 9 = every product, the same
# exact-products / fp32-accumulation contract as the fp32 instruction; 6 = without the three products of relative size <= 2^-24).
# "auto" (default since round 6): six piece products on the shapes where they are BOTH faster and no further from an fp64
# evaluation than the fp32 instruction -- Cin >= AUTO_MIN_CIN (the piece form accumulates 8 / 16 products per rounding, the fp32
# instruction 2: its advantage grows with the contraction length; at Cin = 32 it is 7-11 % further away, profiles/r05/
# kbench_gemm_error.txt) and Cout % 128 == 0 (the block form: A split once per block, 1.5 x the fp32 form's speed) -- the fp32
# instruction everywhere else.  The rule is gated by tests/test_gpu_parity.py::test_auto_gemm_form_is_no_further_from_fp64.
GEMM_PIECES = os.environ.get("EQA_FFT_GEMM_PIECES", "auto")
AUTO_MIN_CIN = int(os.environ.get("EQA_FFT_GEMM_AUTO_MIN_CIN", "128"))
# "h3" (round 6, the default where it applies): TWO fp16 pieces per operand, three exact products per product on the fp16 matrix
# cores (eqa_fft48k5_cgemm3m_f16x2).  Half the matrix instructions of "6" and closer to fp64 than "6" AND the fp32 instruction for
# Cin >= AUTO_MIN_CIN_H3 (fewer accumulator roundings; profiles/r06/kbench_gemm_error.txt) -- but fp16's range wants the operands
# scaled, so it runs only where the producer of V hands over a bound of |V| on the device: the fused lifting kernel on non-negative
# (relu) activations, whose DC bins bound every other bin (eqa_lift5_fft48k5_input_dcmax).  Everywhere else "auto" stays as above.
AUTO_MIN_CIN_H3 = int(os.environ.get("EQA_FFT_GEMM_AUTO_MIN_CIN_H3", "64"))
# Which matrix instruction "h3" runs on: "32" = v_mfma_f32_32x32x16_f16 (eqa_fft48k5_cgemm3m_f16x2, K-stages of 16), "16" =
# v_mfma_f32_16x16x32_f16 (eqa_fft48k5_cgemm3m_f16x2_k32, K-stages of 32: round 27).  Same operands, split and products; the low bits
# of the result differ (32 k per accumulator rounding instead of 16).  The A/B switch of profiles/r27.
H3_MFMA = os.environ.get("EQA_FFT_GEMM_H3_MFMA", "16")
H3_ENTRIES = {"32": ("pieces_f16", "eqa_fft48k5_cgemm3m_f16x2"), "16": ("pieces_f16_k32", "eqa_fft48k5_cgemm3m_f16x2_k32")}   # H3_MFMA -> (Spectra3M's split, the entry)
LAST_H3_MFMA = None     # ... and which of the two the most recent "h3" contraction ran on
DCMAX_SLOTS = 256       # EQA_LIFT5_DCMAX_SLOTS (include/eqa_hip.h)
LAST_FORM = None        # the form the most recent `contract` on the hand-written GEMM ran in (bench.py reports it)
# Channel counts the kernels above do not take but that are multiples of 16 (144 = 16 fields x 9 of the steerable network, 288, 48,
# 80): the same 3-multiplication arithmetic on 64 x 32 wave tiles (eqa_fft48_cgemm3m_c16) and, for the filter gradient, 32 x 32
# channel tiles (eqa_fft48_wgrad3m_c16).  EQA_FFT_GEMM_C16=0: the library's real batched GEMM for both, as before they existed.
GEMM_C16 = os.environ.get("EQA_FFT_GEMM_C16", "1") != "0"
LAST_CONTRACTION = None   # which contraction the most recent `contract` ran: "3m" (eqa_fft48k5_cgemm3m*), "c16", "lib" (torch.bmm)
LAST_WGRAD = None         # ... and the most recent `filter_grad_k`: "3m" (eqa_fft48k5_wgrad3m), "c16", "lib"


def f16_form_takes(cin: int, cout: int) -> bool:
    return cout % 128 == 0 and cin % 32 == 0


def gemm_form(cin: int, cout: int, bounded: bool = False) -> str:
    """"f32" / "9" / "6" / "h3": how `contract` multiplies a (.., 2 cin) . (2 cin, 2 cout) complex product (see GEMM_PIECES).
    ``bounded``: the caller holds an upper bound of |V| on the device (what the fp16 form "h3" needs)."""
    if GEMM_PIECES in ("f32", "9", "6"):
        return GEMM_PIECES
    if bounded and f16_form_takes(cin, cout) and (GEMM_PIECES == "h3" or cin >= AUTO_MIN_CIN_H3):
        return "h3"
    # "auto", and "h3" without a bound or on a shape the fp16 kernel does not take
    return "6" if cin >= AUTO_MIN_CIN and cout % 128 == 0 else "f32"


def f16_scale(t: torch.Tensor) -> float:
    """The power of two that takes max |t| to at most 2^14: what an operand is multiplied by before it is split into fp16 pieces
    (1 for an all-zero or non-finite t).  One host synchronisation when t is on the device."""
    mx = float(t.abs().max().item())
    ex = 14 - math.frexp(mx)[1] if 0.0 < mx < float("inf") else 0        # mx <= 2^frexp(mx)[1]
    return math.ldexp(1.0, max(-100, min(100, ex)))


class Spectra3M:
    """Filter spectra in the operand order of eqa_fft48k5_cgemm3m: ``data`` is the flat (F * Cin * Cout * 3) fp32 buffer
    [Br | Bi | Br + Bi] per (frequency, K-stage, 32 output channels); ``pieces()``: the same split into three bf16 pieces per value
    in the fragment order of the bf16 matrix instruction (built on first use)."""

    __slots__ = ("data", "cin", "cout", "_pieces", "_pieces_f16", "_pieces_f16_k32")

    def __init__(self, data: torch.Tensor, cin: int, cout: int):
        self.data, self.cin, self.cout, self._pieces, self._pieces_f16, self._pieces_f16_k32 = data, cin, cout, None, None, None

    def _split_f16(self, slot: str, entry: str):
        """The (pieces, b_scale) pair kept in ``slot``, split by the library's ``entry`` on first use.  The scale is the other fp16
        form's once that one is built (one host synchronisation for the maximum between the two)."""
        if getattr(self, slot) is None:
            lib = _lib.load()
            built = self._pieces_f16 or self._pieces_f16_k32
            scale = built[1] if built is not None else f16_scale(self.data)
            b = torch.empty(lib.eqa_fft48k5_spectra3m_f16_bytes(self.cin, self.cout) // 2, dtype=torch.int16, device=self.data.device)
            with torch.cuda.device(self.data.device):
                _lib.check(getattr(lib, entry)(self.data.data_ptr(), b.data_ptr(), self.cin, self.cout, scale, ops._stream()), entry)
            setattr(self, slot, (b, scale))
        return getattr(self, slot)

    def pieces_f16(self):
        """(Bh, b_scale): the spectra times the power of two b_scale (max |.| -> at most 2^14) as two fp16 pieces per value, in the
        fragment order of the fp16 matrix instruction (built on first use: one host synchronisation for the maximum)."""
        return self._split_f16("_pieces_f16", "eqa_fft48k5_spectra3m_split_f16")

    def pieces_f16_k32(self):
        """(Bk, b_scale): as `pieces_f16`, in the fragment order of the 16x16x32 instruction (eqa_fft48k5_cgemm3m_f16x2_k32); built
        on first use, the same number of bytes."""
        return self._split_f16("_pieces_f16_k32", "eqa_fft48k5_spectra3m_split_f16_k32")

    def pieces(self) -> torch.Tensor:
        if self._pieces is None:
            lib = _lib.load()
            bp = torch.empty(lib.eqa_fft48k5_spectra3m_bf16_bytes(self.cin, self.cout) // 2, dtype=torch.int16, device=self.data.device)
            with torch.cuda.device(self.data.device):
                _lib.check(lib.eqa_fft48k5_spectra3m_split(self.data.data_ptr(), bp.data_ptr(), self.cin, self.cout,
                                                           ops._stream()), "eqa_fft48k5_spectra3m_split")
            self._pieces = bp
        return self._pieces


def gemm3m_supported(cin: int, cout: int) -> bool:
    return GEMM == "3m" and bool(_lib.load().eqa_fft48k5_cgemm3m_supported(cin, cout))


class Spectra3MC16:
    """Filter spectra in the operand order of eqa_fft48_cgemm3m_c16: ``data`` is the flat fp32 buffer
    (F, Cin/16, ceil(Cout/32), 3 [Br | Bi | Br + Bi], 2, 64, 4) with the columns beyond Cout zero (include/eqa_hip.h).  fp32 only: the
    bf16 / fp16 piece forms do not exist for these channel counts."""

    __slots__ = ("data", "cin", "cout")

    def __init__(self, data: torch.Tensor, cin: int, cout: int):
        self.data, self.cin, self.cout = data, cin, cout

    def unpack(self, pad: bool = False):
        """(Br, Bi, Bs) as (F, Cin, Cout) tensors (``pad``: (F, Cin, 32 ceil(Cout/32)), the padding columns included)."""
        nct = (self.cout + 31) // 32
        t = self.data.view(F, self.cin // 16, nct, 3, 2, 2, 32, 4)             # (f, s, c, part, b, h, j, t)
        t = t.permute(3, 0, 1, 4, 5, 7, 2, 6).reshape(3, F, self.cin, nct * 32)   # k = 16 s + 8 b + 4 h + t; column 32 c + j
        if not pad:
            t = t[..., :self.cout]
        return t[0], t[1], t[2]


def gemm3m_c16_supported(cin: int, cout: int) -> bool:
    """The 16-multiple contraction takes what the kernels above leave to the library."""
    return (GEMM == "3m" and GEMM_C16 and not gemm3m_supported(cin, cout)
            and bool(_lib.load().eqa_fft48_cgemm3m_c16_supported(cin, cout)))


def filter_spectra3m_c16(bank: torch.Tensor, correlate: bool = True) -> Spectra3MC16:
    """(Cout, Cin, k, k) fp32 device bank -> the spectra of `filter_spectra` / `spectra_for_k`, laid out for eqa_fft48_cgemm3m_c16."""
    lib = _lib.load()
    Cout, Cin, k = bank.shape[0], bank.shape[1], bank.shape[-1]
    if not (bank.is_cuda and bank.dtype == torch.float32 and lib.eqa_fft48_cgemm3m_c16_supported(Cin, Cout)):
        raise RuntimeError("filter_spectra3m_c16: fp32 device bank with Cin % 16 == 0 and Cout % 16 == 0 expected")
    B3 = torch.empty(lib.eqa_fft48_spectra3m_c16_floats(Cin, Cout), dtype=torch.float32, device=bank.device)
    with torch.cuda.device(bank.device):
        if k == 5:
            _lib.check(lib.eqa_fft48k5_filter_spectra3m_c16(bank.contiguous().data_ptr(), B3.data_ptr(), Cout, Cin, int(correlate),
                                                            ops._stream()), "eqa_fft48k5_filter_spectra3m_c16")
        else:
            _lib.check(lib.eqa_fft48_filter_spectra3m_c16(bank.contiguous().data_ptr(), B3.data_ptr(), Cout, Cin, k, int(correlate),
                                                          ops._stream()), "eqa_fft48_filter_spectra3m_c16")
    return Spectra3MC16(B3, Cin, Cout)


def filter_spectra3m(bank: torch.Tensor, correlate: bool = True) -> Spectra3M:
    """(Cout, Cin, 5, 5) device bank -> the same spectra as `filter_spectra`, laid out for the 3-multiplication complex GEMM."""
    lib = _lib.load()
    Cout, Cin = bank.shape[:2]
    if not (bank.is_cuda and bank.dtype == torch.float32 and lib.eqa_fft48k5_cgemm3m_supported(Cin, Cout)):
        raise RuntimeError("filter_spectra3m: fp32 device bank with Cin % 32 == 0 and Cout % 64 == 0 expected")
    B3 = torch.empty(lib.eqa_fft48k5_spectra3m_floats(Cin, Cout), dtype=torch.float32, device=bank.device)
    with torch.cuda.device(bank.device):
        _lib.check(lib.eqa_fft48k5_filter_spectra3m(bank.contiguous().data_ptr(), B3.data_ptr(), Cout, Cin, int(correlate),
                                                    ops._stream()), "eqa_fft48k5_filter_spectra3m")
    return Spectra3M(B3, Cin, Cout)


def spectra_for(bank: torch.Tensor, correlate: bool = True):
    """The filter spectra in the form the contraction will consume: `Spectra3M` where the hand-written GEMM takes the channel
    counts, else the (F, 2Cin, 2Cout) real form for the library GEMM."""
    Cout, Cin = bank.shape[:2]
    if bank.is_cuda and bank.dtype == torch.float32 and gemm3m_supported(Cin, Cout):
        return filter_spectra3m(bank, correlate)
    if bank.is_cuda and bank.dtype == torch.float32 and gemm3m_c16_supported(Cin, Cout):
        return filter_spectra3m_c16(bank, correlate)
    return filter_spectra(bank, correlate=correlate)


def contract(V: torch.Tensor, B, M: int, vbound: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Mo[f] = V[f] . B[f] for every stored frequency: V (F, M, 2Cin) view of a pitched buffer -> Mo (F, M, 2Cout) likewise.
    ``vbound``: a device fp32 tensor whose maximum bounds every |Re|, |Im| of V (the producer's DC bins) -- admits the fp16 form."""
    dev = V.device
    global LAST_FORM, LAST_CONTRACTION, LAST_H3_MFMA
    if isinstance(B, Spectra3MC16):
        lib = _lib.load()
        assert V.shape[2] == 2 * B.cin and V.stride(1) == 2 * B.cin and V.stride(0) == lib.eqa_fft48k5_tile_pitch(M) * 2 * B.cin
        Mo = spectra_buffer(M, 2 * B.cout, dev)
        LAST_CONTRACTION = "c16"
        _lib.check(lib.eqa_fft48_cgemm3m_c16(V.data_ptr(), B.data.data_ptr(), Mo.data_ptr(), M, B.cin, B.cout, ops._stream()),
                   "eqa_fft48_cgemm3m_c16")
        return Mo
    if isinstance(B, Spectra3M):
        lib = _lib.load()
        assert V.shape[2] == 2 * B.cin and V.stride(1) == 2 * B.cin and V.stride(0) == lib.eqa_fft48k5_tile_pitch(M) * 2 * B.cin
        Mo = spectra_buffer(M, 2 * B.cout, dev)
        LAST_CONTRACTION = "3m"
        form = LAST_FORM = gemm_form(B.cin, B.cout, vbound is not None)
        if form == "h3":
            if H3_MFMA not in H3_ENTRIES:
                raise RuntimeError(f"EQA_FFT_GEMM_H3_MFMA: \"16\" or \"32\" expected, not {H3_MFMA!r}")
            LAST_H3_MFMA = H3_MFMA
            pieces, entry = H3_ENTRIES[H3_MFMA]
            bh, b_scale = getattr(B, pieces)()
            _lib.check(getattr(lib, entry)(V.data_ptr(), bh.data_ptr(), Mo.data_ptr(), M, B.cin, B.cout, vbound.data_ptr(),
                                           vbound.numel(), b_scale, ops._stream()), entry)
            return Mo
        if form in ("9", "6"):
            _lib.check(lib.eqa_fft48k5_cgemm3m_bf16x3(V.data_ptr(), B.pieces().data_ptr(), Mo.data_ptr(), M, B.cin, B.cout, int(form),
                                                      ops._stream()), "eqa_fft48k5_cgemm3m_bf16x3")
            return Mo
        _lib.check(lib.eqa_fft48k5_cgemm3m(V.data_ptr(), B.data.data_ptr(), Mo.data_ptr(), M, B.cin, B.cout,
                                           ops._stream()), "eqa_fft48k5_cgemm3m")
        return Mo
    LAST_CONTRACTION = "lib"
    return torch.bmm(V, B, out=spectra_buffer(M, B.shape[2], dev))


def freq_index():
    """(ky, kx) of stored frequency f, in the kernels' order: f = 23 ky + kx - 1 for 0 < kx < 24 (all 48 ky), then
    1104 + 2 ky + (kx == 24) for the edge columns, ky <= 24."""
    ky = torch.arange(N).repeat_interleave(NH - 2)
    kx = torch.arange(1, NH - 1).repeat(N)
    eky = torch.arange(NH).repeat_interleave(2)
    ekx = torch.tensor([0, NH - 1]).repeat(NH)
    return torch.cat([ky, eky]), torch.cat([kx, ekx])


def tiles_k(n: int, k: int) -> int:
    """Tiles along an axis of n input pixels for a k x k kernel: 49 - k outputs each."""
    o = N + 1 - k
    return 0 if n < k else (n - (k - 1) + o - 1) // o


def tiles(n: int) -> int:
    return tiles_k(n, 5)


def _stands_for_channels_last(self, memory_format=torch.contiguous_format) -> bool:
    """`is_contiguous` of `GroupedMap` / `LiftedInput`: that of the tensor they turn into when no FFT layer takes them, so that a
    consumer's applicability rule can be asked before anything is written."""
    return memory_format == torch.channels_last


class GroupedMap:
    """An activation map in the channel-group-major layout (nimg, C/16, H, W, 16) written by `ops.lift_conv_grouped` and read by
    `conv5x5` (eqa_fft48k5_input_grouped): `.shape` is the logical (nimg, C, H, W)."""

    def __init__(self, data: torch.Tensor):
        assert data.dim() == 5 and data.shape[-1] == 16 and data.is_contiguous()
        self.data = data
        self.shape = torch.Size((data.shape[0], data.shape[1] * 16, data.shape[2], data.shape[3]))
        self.device, self.dtype, self.is_cuda = data.device, data.dtype, data.is_cuda

    def data_ptr(self) -> int:
        return self.data.data_ptr()

    def to_channels_last(self) -> torch.Tensor:
        """The same map as an ordinary channels-last (nimg, C, H, W) tensor (a copy)."""
        n, g, h, w, _ = self.data.shape
        return self.data.permute(0, 1, 4, 2, 3).reshape(n, g * 16, h, w).contiguous(memory_format=torch.channels_last)

    materialize, is_contiguous = to_channels_last, _stands_for_channels_last


class LiftedInput:
    """A lifting layer that has NOT run: (x channels-last (nimg, 3, H0, W0), folded 5 x 5 bank (C, 3, 5, 5) channels-last, bias (C),
    relu) standing for the map [relu](conv2d(x, bank) + bias) of logical `.shape` (nimg, C, H0 - 4, W0 - 4).  `conv5x5` takes it in
    place of that map and produces the map's tile spectra straight from x (eqa_lift5_fft48k5_input: the lifting convolution fused
    into the forward FFT-48 transform -- the 2.2 GB map of the headline shape is neither written nor read)."""

    def __init__(self, x: torch.Tensor, bank: torch.Tensor, bias: Optional[torch.Tensor], relu: bool, pieces: Optional[torch.Tensor] = None,
                 pieces_f16=None):
        assert x.dim() == 4 and x.shape[1] == 3 and bank.shape[1:] == (3, 5, 5)
        self.x = x.contiguous(memory_format=torch.channels_last)
        self.bank = bank.contiguous(memory_format=torch.channels_last)           # memory order (C, 5, 5, 3)
        self.bias, self.relu = (bias.contiguous() if bias is not None else None), bool(relu)
        self.shape = torch.Size((x.shape[0], bank.shape[0], x.shape[2] - 4, x.shape[3] - 4))
        self.device, self.dtype, self.is_cuda = x.device, x.dtype, x.is_cuda
        self._pieces = pieces
        self._pieces_f16 = pieces_f16
        self.bound_route: Optional[str] = None      # where `spectra_into` took the pixels' bound from, once it has run

    @staticmethod
    def split_f16(bank: torch.Tensor):
        """(wh, w_scale): a folded bank as the operand of eqa_lift5_fft48k5_input_f16x2 -- (C, 2 pieces, 5 filter rows, 4 chunks, 8)
        fp16 of w_scale * w (w_scale: `f16_scale`); chunk p < 3 of filter row ky =
        [w(ci 0..2, kx = 2 p - 1), 0, w(ci 0..2, kx = 2 p), 0] (kx = -1: 0), chunk 3 = 0; pieces h1 = rn16(v), h2 = rn16(v - h1).
        One host synchronisation; the network caches it per weight version."""
        w = bank.float()                                        # (C, 3, 5, 5) logical
        C = w.shape[0]
        scale = f16_scale(w)
        wp = torch.zeros(C, 5, 8, 4, dtype=torch.float32, device=w.device)       # (co, ky, kx + 1 in 0..7, ci padded to 4)
        wp[:, :, 1:6, :3] = w.permute(0, 2, 3, 1) * scale
        chunks = wp.reshape(C, 5, 4, 8)
        h1 = chunks.half()
        h2 = (chunks - h1.float()).half()
        return torch.stack([h1, h2], dim=1).contiguous(), scale

    @staticmethod
    def split_bf16(bank: torch.Tensor) -> torch.Tensor:
        """A folded bank as the operand of eqa_lift5_fft48k5_input_bf16x3: (C, 3 pieces, 16 chunks, 8) bf16 -- chunk c < 15 = (filter
        row c // 3, pixel pair c % 3): [w(ci 0..2, kx = 2 p), 0, w(ci 0..2, kx = 2 p + 1), 0] (kx = 5: 0), chunk 15 = 0; every value
        split exactly into three bf16 pieces (the network caches it per weight version)."""
        w = bank.float()                                        # (C, 3, 5, 5) logical
        C = w.shape[0]
        wp = torch.zeros(C, 5, 6, 4, dtype=torch.float32, device=w.device)       # (co, ky, kx padded to 6, ci padded to 4)
        wp[:, :, :5, :3] = w.permute(0, 2, 3, 1)
        chunks = torch.zeros(C, 16, 8, dtype=torch.float32, device=w.device)
        chunks[:, :15] = wp.reshape(C, 5, 3, 8).reshape(C, 15, 8)
        p0 = chunks.bfloat16()
        r1 = chunks - p0.float()
        p1 = r1.bfloat16()
        p2 = (r1 - p1.float()).bfloat16()
        assert torch.equal((p0.float() + p1.float()) + p2.float(), chunks), "the three bf16 pieces of a weight must add up exactly"
        return torch.stack([p0, p1, p2], dim=1).contiguous()

    @classmethod
    def form_operand(cls):
        """(cache tag, constructor keyword, builder from the folded bank) of the packed filter operand that the fused kernel reads in
        the form LIFT_FFT_FORM names, for a caller that keeps it across LiftedInputs; None: the form reads the bank itself."""
        return {"h2": ("lifth", "pieces_f16", cls.split_f16), "bf16x3": ("liftp", "pieces", cls.split_bf16)}.get(LIFT_FFT_FORM)

    def pieces_f16(self):
        """`split_f16` of this bank, built once per LiftedInput unless handed in."""
        if self._pieces_f16 is None:
            self._pieces_f16 = self.split_f16(self.bank)
        return self._pieces_f16

    def pieces(self) -> torch.Tensor:
        """`split_bf16` of this bank, built once per LiftedInput unless handed in."""
        if self._pieces is None:
            self._pieces = self.split_bf16(self.bank)
        return self._pieces

    def spectra_into(self, V: torch.Tensor, B, st: int) -> Optional[torch.Tensor]:
        """Write the tile spectra of the map this stands for into V (F, M, 2C), in the arithmetic LIFT_FFT_FORM names, on stream st.
        Returns DCMAX_SLOTS floats whose maximum bounds |V| where the contraction with the spectra B will use them (non-negative
        activations and the fp16 form "h3": the kernel hands over its DC bins), else None."""
        lib = _lib.load()
        nimg, C, H, W = self.shape
        dims = (nimg, H + 4, W + 4, C, st)
        px, pV = self.x.data_ptr(), V.data_ptr()
        p_b = self.bias.data_ptr() if self.bias is not None else None
        want_dc = self.relu and isinstance(B, Spectra3M) and gemm_form(B.cin, B.cout, True) == "h3"
        vbound = None
        if LIFT_FFT_FORM == "h2" and px % 16 == 0:      # (eqa_absmax_slots reads 16 bytes per lane)
            wh, w_scale = self.pieces_f16()
            xbound = ops.crop_absmax_slots(self.x)      # the resize kernel's, while nothing has written to x since
            self.bound_route = "crop_slots" if xbound is not None else "eqa_absmax_slots"
            if xbound is None:
                xbound = torch.empty(DCMAX_SLOTS, dtype=torch.float32, device=self.device)
                _lib.check(lib.eqa_absmax_slots(px, self.x.numel(), xbound.data_ptr(), st), "eqa_absmax_slots")
            if want_dc:
                vbound = torch.empty(DCMAX_SLOTS, dtype=torch.float32, device=self.device)
            _lib.check(lib.eqa_lift5_fft48k5_input_f16x2(px, wh.data_ptr(), w_scale, xbound.data_ptr(), xbound.numel(), p_b, int(self.relu), pV,
                                                         vbound.data_ptr() if want_dc else None, *dims), "eqa_lift5_fft48k5_input_f16x2")
        elif LIFT_FFT_FORM == "bf16x3":                 # (this form has no variant that hands the DC bins over)
            _lib.check(lib.eqa_lift5_fft48k5_input_bf16x3(px, self.pieces().data_ptr(), p_b, int(self.relu), pV, *dims),
                       "eqa_lift5_fft48k5_input_bf16x3")
        elif want_dc:
            vbound = torch.empty(DCMAX_SLOTS, dtype=torch.float32, device=self.device)
            _lib.check(lib.eqa_lift5_fft48k5_input_dcmax(px, self.bank.data_ptr(), p_b, 1, pV, vbound.data_ptr(), *dims),
                       "eqa_lift5_fft48k5_input_dcmax")
        else:
            _lib.check(lib.eqa_lift5_fft48k5_input(px, self.bank.data_ptr(), p_b, int(self.relu), pV, *dims), "eqa_lift5_fft48k5_input")
        return vbound

    def materialize(self) -> torch.Tensor:
        """The map itself, channels-last (the unfused lifting kernel) -- for a consumer that turned out not to be `conv5x5`."""
        return ops.lift_conv_nhwc(self.x, ops.pack_lift_weights(self.bank), self.bias, self.relu, 5, 5)

    is_contiguous = _stands_for_channels_last


# how the fused kernel multiplies: "h2" (default since the end of round 6) = two fp16 pieces per value, three exact products on the fp16
# matrix cores (eqa_lift5_fft48k5_input_f16x2; pixels scaled under the bound eqa_absmax_slots takes, one 10 us launch; as close to
# fp64 as the fp32 form: tests/test_gpu_lift_fft.py), "f32" = v_mfma_f32_16x16x4_f32 (which shares the vector ALU's datapath with the
# transforms), "bf16x3" = exact three-piece splits, six products on the bf16 matrix cores (opt-in: no faster than f32)
LIFT_FFT_FORM = os.environ.get("EQA_LIFT_FFT_FORM", "h2")
LIFT_FFT_FUSED_DEFAULT = "1"     # EQA_LIFT_FFT_FUSED=0: the two kernels (eqa_lift_conv_grouped, eqa_fft48k5_input_grouped)


def lift_fused_applicable(x_shape, bank_shape, cout_next: int, device) -> bool:
    """Can the lifting layer (x_shape channels-last input, bank_shape (C, Cin, k, k)) be fused into the FFT convolution behind it?"""
    if os.environ.get("EQA_LIFT_FFT_FUSED", LIFT_FFT_FUSED_DEFAULT) == "0" or len(x_shape) != 4:
        return False
    C, Cin, kh, kw = bank_shape
    if not _lib.load().eqa_lift5_fft48k5_input_supported(Cin, kh, kw, C):
        return False
    out_shape = (x_shape[0], C, x_shape[2] - 4, x_shape[3] - 4)
    return x_shape[2] >= 5 and x_shape[3] >= 5 and grouped_applicable(out_shape, C, cout_next, device)


def _tiles_pay(shape, cin: int, cout: int, max_waste: float) -> bool:
    """What `applicable` and `grouped_applicable` share: a contraction that is ours to run, enough tiles to amortise the filter spectra
    (``MIN_TILES``), and tiles that fit the output to within ``max_waste`` (the FFT work is per tile: 88 outputs per axis = 2 tiles
    exactly, 84 would waste 5 %, 50 would waste 43 % -> Winograd)."""
    if shape[1] != cin or (not gemm3m_supported(cin, cout) and ops.plane_gemm_supported(cin, cout)):
        # (e.g. 32 output channels: the complex GEMM wants 64-column tiles, the Winograd planes' GEMM takes 32 -- the path whose
        # contraction is hand-written wins over the one that would call the library)
        return False
    H, W = shape[-2:]
    if H < 16 or W < 16 or shape[0] * tiles(H) * tiles(W) < MIN_TILES:
        return False
    return tiles(H) * OUT <= max_waste * (H - 4) and tiles(W) * OUT <= max_waste * (W - 4)


def grouped_applicable(shape, cin: int, cout: int, device, max_waste: float = 1.12) -> bool:
    """Would `conv5x5` take a (nimg, cin, H, W) fp32 map of this shape on `device` through the FFT path AND read it in the
    grouped layout?  (Decided before the producing layer runs, so that it can write that layout.)"""
    if not (ENABLED and device.type == "cuda" and len(shape) == 4 and cin % 16 == 0):
        return False
    if os.environ.get("EQA_FFT_GROUPED", "1") == "0" or not _lib.load().eqa_fft48k5_input_grouped_supported(cin):
        return False
    return _tiles_pay(shape, cin, cout, max_waste)


def applicable(x: torch.Tensor, cin: int, cout: int, max_waste: float = 1.12) -> bool:
    """Should `conv5x5` take x: a channels-last fp32 device tensor (or a map standing in its place) that `_tiles_pay`."""
    if isinstance(x, (GroupedMap, LiftedInput)):
        return grouped_applicable(x.shape, cin, cout, x.device, max_waste)
    if not (ENABLED and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    return _tiles_pay(x.shape, cin, cout, max_waste)


def _order(C: int, G: int) -> torch.Tensor:
    """Position p of a 2C-wide row -> index into [Re(0..C-1), Im(0..C-1)]: groups of G channels, [Re x G | Im x G] each."""
    p = torch.arange(2 * C)
    grp, r = p // (2 * G), p % (2 * G)
    return (r // G) * C + grp * G + r % G


def group_sizes(cin: int, cout: int):
    """Channels per [Re | Im] group in the rows of V (16: what a block of the fused forward kernel owns) and of Mo (1)."""
    return (16 if cin % 16 == 0 else 1), 1


def filter_spectra(bank: torch.Tensor, groups=None, correlate: bool = True) -> torch.Tensor:
    """(Cout, Cin, 5, 5) -> B:(F, 2 Cin, 2 Cout) fp32, the real form of conj(FFT(filter)) / 48^2 per frequency.  Rows
    follow the rows of V, columns the rows of Mo (``group_sizes``; ``groups`` = (Cin, Cout) gives the plain [Re | Im] order)."""
    Cout, Cin = bank.shape[:2]
    if groups is None and bank.is_cuda and bank.dtype == torch.float32:
        lib = _lib.load()                                         # on the device: one kernel (eqa_fft48k5_filter_spectra)
        B = torch.empty((F, 2 * Cin, 2 * Cout), dtype=torch.float32, device=bank.device)
        with torch.cuda.device(bank.device):
            _lib.check(lib.eqa_fft48k5_filter_spectra(bank.contiguous().data_ptr(), B.data_ptr(), Cout, Cin, int(correlate),
                                                      ops._stream()), "eqa_fft48k5_filter_spectra")
        return B
    assert correlate, "the host construction is the correlation (forward) form"
    gin, gout = groups if groups is not None else group_sizes(Cin, Cout)
    wp = torch.zeros(Cout, Cin, N, N, dtype=torch.float64, device=bank.device)
    wp[:, :, :5, :5] = bank.double()
    W = torch.fft.rfft2(wp).conj() / float(N * N)                # (Cout, Cin, 48, 25)
    ky, kx = freq_index()
    W = W[:, :, ky.to(W.device), kx.to(W.device)]                # (Cout, Cin, F)
    Wr = W.real.permute(2, 1, 0).contiguous()
    Wi = W.imag.permute(2, 1, 0).contiguous()
    top = torch.cat([Wr, Wi], dim=2)                              # rows Re(A): [ Br |  Bi ]
    bot = torch.cat([-Wi, Wr], dim=2)                             # rows Im(A): [-Bi |  Br ]
    full = torch.cat([top, bot], dim=1)                           # rows [Re ci | Im ci], columns [Re co | Im co]
    full = full[:, _order(Cin, gin).to(bank.device)][:, :, _order(Cout, gout).to(bank.device)]
    return full.float().contiguous()


def spectra_buffer(M: int, width: int, device) -> torch.Tensor:
    """(F, M, width) fp32 view of a buffer with eqa_fft48k5_tile_pitch(M) = M | 1 rows per frequency -- the layout every
    eqa_fft48k5_* entry point reads and writes (an even tile count such as 1024 would put all the frequencies of a tile
    into the same HBM channel).  The batched GEMMs run on the view; the padding row is never touched."""
    pitch = _lib.load().eqa_fft48k5_tile_pitch(M)
    return torch.empty((F, pitch, width), dtype=torch.float32, device=device)[:, :M]


def output_stats_supported(nimg: int, OH: int, OW: int, cout: int) -> bool:
    """The inverse transform can take the batch-norm statistics of its output on the way out (eqa_fft48k5_output_stats)."""
    return _lib.load().eqa_fft48k5_output_stats_rows(nimg, OH, OW, cout) > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# Kernel sizes other than 5 (round 4): the same scheme with O = 49 - k outputs per tile, through eqa_fft48_* (two-pass kernels).
# The reference's kernel_size is a free constructor argument (escnn_networks.py:19-44): its tutorial trains k = 9, its test k = 3.
# k = 5 keeps kernels of its own (eqa_fft48k5_*: fused / pipelined transforms, the window-sum / statistics epilogues, the grouped and
# fused-lifting inputs).  The transforms of the two families take the same arguments but for k, which `_transform` / `_workspace` add.
# ----------------------------------------------------------------------------------------------------------------------------------
KSIZES = (3, 5, 7, 9)


def _transform(name: str, k: int, *args) -> None:
    """Launch eqa_fft48k5_<name>(*args) for k = 5, eqa_fft48_<name>(..., k, stream) otherwise (args end with the stream)."""
    lib = _lib.load()
    if k == 5:
        _lib.check(getattr(lib, "eqa_fft48k5_" + name)(*args), "eqa_fft48k5_" + name)
    else:
        _lib.check(getattr(lib, "eqa_fft48_" + name)(*args[:-1], k, args[-1]), "eqa_fft48_" + name)


def _workspace(k: int, nimg: int, rows: int, out_cols: int, C: int, device) -> torch.Tensor:
    """The scratch buffer a transform over (nimg, rows, out_cols, C) asks for."""
    lib = _lib.load()
    nbytes = lib.eqa_fft48k5_workspace_bytes(nimg, rows, out_cols, C) if k == 5 else lib.eqa_fft48_workspace_bytes(nimg, rows, out_cols, C, k)
    return torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=device)


def applicable_k(x_shape, cin: int, cout: int, k: int, device, channels_last: bool = True) -> bool:
    """Should a (nimg, cin, H, W) fp32 channels-last map on `device` take the FFT path for a k x k stride-1 convolution?
    k = 5: the tuned rule above (`applicable`).  Otherwise a cost model -- the FFT path moves ~2.2 x its spectra (two-pass
    transforms) at ~4 TB/s and contracts 1154 x 3 real products per tile and channel pair at ~100 TFLOP/s; the library's
    direct convolution runs its OH x OW x k^2 products at ~110 TFLOP/s -- with a 1.3 x margin in favour of the library."""
    if not (ENABLED and k in KSIZES and k != 5 and device.type == "cuda" and channels_last and len(x_shape) == 4 and x_shape[1] == cin):
        return False
    if os.environ.get("EQA_FFT_ANYK", "1") == "0":
        return False
    nimg, _, H, W = x_shape
    if H < max(16, k) or W < max(16, k) or nimg * tiles_k(H, k) * tiles_k(W, k) < 8:
        return False
    oh, ow = H - k + 1, W - k + 1
    t = tiles_k(H, k) * tiles_k(W, k)
    fft_us = t * (F * 8 * (cin + cout) * 2.2 / 4.0e6 + F * 6 * cin * cout / 100e6)
    direct_us = oh * ow * k * k * 2 * cin * cout / 110e6
    return fft_us * 1.3 < direct_us


def spectra_for_k(bank: torch.Tensor, correlate: bool = True):
    """`spectra_for` for a (Cout, Cin, k, k) device bank of any supported k."""
    k = bank.shape[-1]
    if k == 5:
        return spectra_for(bank, correlate)
    lib = _lib.load()
    Cout, Cin = bank.shape[:2]
    assert bank.is_cuda and bank.dtype == torch.float32 and bank.shape[-2] == k and lib.eqa_fft48_supported(k)
    st = ops._stream()
    with torch.cuda.device(bank.device):
        if gemm3m_supported(Cin, Cout):
            B3 = torch.empty(lib.eqa_fft48k5_spectra3m_floats(Cin, Cout), dtype=torch.float32, device=bank.device)
            _lib.check(lib.eqa_fft48_filter_spectra3m(bank.contiguous().data_ptr(), B3.data_ptr(), Cout, Cin, k, int(correlate), st),
                       "eqa_fft48_filter_spectra3m")
            return Spectra3M(B3, Cin, Cout)
        if gemm3m_c16_supported(Cin, Cout):
            return filter_spectra3m_c16(bank, correlate)
        B = torch.empty((F, 2 * Cin, 2 * Cout), dtype=torch.float32, device=bank.device)
        _lib.check(lib.eqa_fft48_filter_spectra(bank.contiguous().data_ptr(), B.data_ptr(), Cout, Cin, k, int(correlate), st),
                   "eqa_fft48_filter_spectra")
        return B


def conv_kxk(x: torch.Tensor, B, k: int, bias: Optional[torch.Tensor], relu: bool, in_bias: Optional[torch.Tensor] = None,
             in_relu: bool = False, keep_V: Optional[list] = None, sums_k: int = 0, stats: Optional[list] = None, tail=None) -> torch.Tensor:
    """x: channels-last (nimg,Cin,H,W) -> channels-last (nimg,Cout,H-k+1,W-k+1) = [relu](conv2d(act(x), g) + bias) with
    B = spectra_for_k(g) (either form) and act(x) = [relu](x + in_bias[c]) applied while loading.
    ``keep_V``: a list that receives the input spectra V (training: the filter gradient reuses them).
    k = 5 only (`conv5x5`): x may be a `GroupedMap` or a `LiftedInput`; ``sums_k`` > 0: return instead the (nimg, Cout, sums_k, sums_k)
    fp64 window sums of that output (the linearised last layer consumes only those), or, with ``tail`` = the operands
    `pooling.sums_tail_operands` built, what the whole tail makes of them in one launch on the inverse transform's partials:
    (activations, index, rotation, reflection) of `ops.window_sums_tail`; ``stats``: a list that receives the
    (rows, Cout, 2) fp64 partial sums of the output's per-channel sum / sum of squares, taken by the inverse transform (training,
    no bias / activation; the caller checks ``output_stats_supported``)."""
    lib = _lib.load()
    nimg, Cin, H, W = x.shape
    if isinstance(B, (Spectra3M, Spectra3MC16)):
        Cout = B.cout
        assert B.cin == Cin
    else:
        Cout = B.shape[2] // 2
        assert B.shape == (F, 2 * Cin, 2 * Cout)
    assert k == 5 or not (sums_k or stats is not None or isinstance(x, (GroupedMap, LiftedInput))), "k = 5 only"
    OH, OW = H - k + 1, W - k + 1
    TX = tiles_k(W, k)
    M = nimg * tiles_k(H, k) * TX
    dev = x.device
    st = ops._stream()
    V = spectra_buffer(M, 2 * Cin, dev)
    p_bias = bias.data_ptr() if bias is not None else None
    vbound = None
    with torch.cuda.device(dev):
        if isinstance(x, LiftedInput):
            assert in_bias is None and not in_relu
            with _timed("lift_fft_input"):
                vbound = x.spectra_into(V, B, st)
        else:
            T = _workspace(k, nimg, H, OW, Cin, dev)
            with _timed("fft_input"):
                _transform("input_grouped" if isinstance(x, GroupedMap) else "input", k, x.data_ptr(), T.data_ptr(), V.data_ptr(),
                           in_bias.data_ptr() if in_bias is not None else None, int(in_relu), nimg, H, W, Cin, st)
            del T
        with _timed("fft_gemm"):
            Mo = contract(V, B, M, vbound)
        if keep_V is not None:
            keep_V.append(V)
        del V
        T2 = _workspace(k, nimg, OH, OW, Cout, dev)
        if sums_k:
            ws = torch.empty(nimg * OH * TX * Cout * (2 * sums_k - 1), dtype=torch.float32, device=dev)
            if tail is not None:
                nseg_sub = (ctypes.c_int * 2)()
                with _timed("fft_output_partials"):
                    _lib.check(lib.eqa_fft48k5_output_sums_partials(Mo.data_ptr(), T2.data_ptr(), p_bias, int(relu), ws.data_ptr(), nimg, OH, OW,
                                                                    Cout, sums_k, nseg_sub, st), "eqa_fft48k5_output_sums_partials")
                return ops.window_sums_tail(ws, nimg, Cout, sums_k, nseg_sub[0], nseg_sub[1], *tail)
            S = torch.empty((nimg, Cout, sums_k, sums_k), dtype=torch.float64, device=dev)
            with _timed("fft_output_sums"):
                _lib.check(lib.eqa_fft48k5_output_sums(Mo.data_ptr(), T2.data_ptr(), p_bias, int(relu), S.data_ptr(), ws.data_ptr(),
                                                       nimg, OH, OW, Cout, sums_k, st), "eqa_fft48k5_output_sums")
            return S
        y = torch.empty((nimg, Cout, OH, OW), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        if stats is not None:
            assert bias is None and not relu
            part = torch.empty((lib.eqa_fft48k5_output_stats_rows(nimg, OH, OW, Cout), Cout, 2), dtype=torch.float64, device=dev)
            with _timed("fft_output"):
                _lib.check(lib.eqa_fft48k5_output_stats(Mo.data_ptr(), T2.data_ptr(), y.data_ptr(), part.data_ptr(), nimg, OH, OW, Cout, st),
                           "eqa_fft48k5_output_stats")
            stats.append(part)
            return y
        with _timed("fft_output"):
            _transform("output", k, Mo.data_ptr(), T2.data_ptr(), p_bias, int(relu), y.data_ptr(), nimg, OH, OW, Cout, st)
        return y


def conv5x5(x: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor], relu: bool,
            in_bias: Optional[torch.Tensor] = None, in_relu: bool = False, sums_k: int = 0,
            keep_V: Optional[list] = None, stats: Optional[list] = None, tail=None) -> torch.Tensor:
    """`conv_kxk` at k = 5, B = spectra_for(g): channels-last (nimg,Cin,H,W), a `GroupedMap` or a `LiftedInput` -> channels-last
    (nimg,Cout,H-4,W-4), or its window sums (``sums_k``) or what the tail makes of them (``tail``), or the map and its batch-norm
    statistics (``stats``)."""
    return conv_kxk(x, B, 5, bias, relu, in_bias, in_relu, keep_V, sums_k, stats, tail)


def grad_spectra(dy: torch.Tensor, k: int = 5) -> torch.Tensor:
    """Spectra of the disjoint (49 - k) x (49 - k) tiles of an output gradient (channels-last), (F, M, 2 Cout): shared by the filter
    gradient and the input gradient."""
    nimg, Cout, OH, OW = dy.shape
    M = nimg * tiles_k(OH + k - 1, k) * tiles_k(OW + k - 1, k)
    T = _workspace(k, nimg, OH, OW, Cout, dy.device)
    G = spectra_buffer(M, 2 * Cout, dy.device)
    with torch.cuda.device(dy.device):
        _transform("grad_transform", k, dy.data_ptr(), T.data_ptr(), G.data_ptr(), nimg, OH, OW, Cout, ops._stream())
    return G


def wgrad_c16_admitted(M: int, cin: int, cout: int) -> bool:
    """Does the filter gradient's contraction over M tiles run eqa_fft48_wgrad3m_c16 rather than the library's GEMM?  Its 32 x 32
    channel tiles do pad32(cin) pad32(cout) / (cin cout) times the work, and the three-product form saves a quarter: admitted where
    that ratio is below 4/3 (96, 112, 144, 288 channels: 1.09 - 1.3 x the library at M = 1024, up to 3.9 x below).  With more padding
    (48 x 48, 48 x 80, 80 x 80: 1.44 - 1.78) it ties with or loses to the library from 512 tiles up and wins only where the library's
    batched GEMM is far from its rate: admitted up to 72 tiles from 48 channels (16 x 16 at M = 1024: 0.105 against 0.067 ms).
    Measured: DESIGN.md section 1, profiles/cgemm3m_c16/."""
    if not (GEMM_C16 and _lib.load().eqa_fft48_wgrad3m_c16_supported(cin, cout)):
        return False
    pad = (-(-cin // 32) * 32) * (-(-cout // 32) * 32)
    return 3 * pad < 4 * cin * cout or (M <= 72 and min(cin, cout) >= 48)


def filter_grad_k(V: torch.Tensor, dy: torch.Tensor, cin: int, k: int, G: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d loss / d filter bank (Cout, Cin, k, k) of y = conv2d(x, bank) from V = the spectra of x's tiles (``keep_V`` of the
    forward pass) and the output gradient dy (channels-last): spectra of the disjoint gradient tiles, one batched GEMM
    over the tiles per frequency (D[f] = V[f]^T G[f]), and the inverse transform restricted to the k x k support
    (eqa_fft48k5_grad_transform / _filter_grad).  2.5 multiplies per output at k = 5 as in the forward pass; Winograd's filter
    gradient (`winograd.filter_grad`) needs 4 and a 4x larger transformed gradient."""
    lib = _lib.load()
    nimg, Cout, OH, OW = dy.shape
    dev = dy.device
    M = V.shape[1]
    assert V.shape == (F, M, 2 * cin) and M == nimg * tiles_k(OH + k - 1, k) * tiles_k(OW + k - 1, k)
    st = ops._stream()
    if G is None:
        G = grad_spectra(dy, k)
    dbank = torch.empty((Cout, cin, k, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        global LAST_WGRAD
        wgrad3m = GEMM == "3m" and os.environ.get("EQA_FFT_WGRAD3M", "1") != "0"
        LAST_WGRAD = ("3m" if wgrad3m and lib.eqa_fft48k5_wgrad3m_supported(cin, Cout) else
                      "c16" if wgrad3m and wgrad_c16_admitted(M, cin, Cout) else "lib")
        packed = LAST_WGRAD != "lib"
        if packed:
            # the contraction over the tiles in the 3-multiplication form on the fp32 MFMA (the library's real GEMM: 4 products)
            D = torch.empty((F, cin, 2, Cout), dtype=torch.float32, device=dev)      # Dr | Di per input channel
            if LAST_WGRAD == "3m":
                _lib.check(lib.eqa_fft48k5_wgrad3m(V.data_ptr(), G.data_ptr(), D.data_ptr(), M, cin, Cout, st), "eqa_fft48k5_wgrad3m")
            else:
                _lib.check(lib.eqa_fft48_wgrad3m_c16(V.data_ptr(), G.data_ptr(), D.data_ptr(), M, cin, Cout, st), "eqa_fft48_wgrad3m_c16")
        else:
            D = torch.bmm(V.transpose(1, 2), G)                   # (F, 2 Cin, 2 Cout)
        if k != 5:                                                # (one entry point, told which D it reads)
            _lib.check(lib.eqa_fft48_filter_grad(D.data_ptr(), dbank.data_ptr(), Cout, cin, k, int(packed), st), "eqa_fft48_filter_grad")
        elif packed:
            _lib.check(lib.eqa_fft48k5_filter_grad3m(D.data_ptr(), dbank.data_ptr(), Cout, cin, st), "eqa_fft48k5_filter_grad3m")
        else:
            _lib.check(lib.eqa_fft48k5_filter_grad(D.data_ptr(), dbank.data_ptr(), Cout, cin, st), "eqa_fft48k5_filter_grad")
    return dbank


def filter_grad(V: torch.Tensor, dy: torch.Tensor, cin: int, G: Optional[torch.Tensor] = None) -> torch.Tensor:
    return filter_grad_k(V, dy, cin, 5, G)


def input_grad(dy: torch.Tensor, bank: torch.Tensor, G: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d loss / d x (channels-last (nimg, Cin, OH+k-1, OW+k-1)) of y = conv2d(x, bank): the full convolution of dy with the
    filters, tile by tile in the frequency domain with overlap-add (eqa_fft48k5_input_grad).  ``G``: the gradient-tile
    spectra if the caller already has them (`grad_spectra`)."""
    k = bank.shape[-1]
    nimg, Cout, OH, OW = dy.shape
    Cin = bank.shape[1]
    dev = dy.device
    if G is None:
        G = grad_spectra(dy, k)
    B2 = spectra_for_k(bank.detach().permute(1, 0, 2, 3).contiguous(), correlate=False)       # spectra of (Cin, Cout, k, k)
    st = ops._stream()
    H, W = OH + k - 1, OW + k - 1
    dx = torch.empty((nimg, Cin, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    with torch.cuda.device(dev):
        Cg = contract(G, B2, G.shape[1])                                          # (F, M, 2 Cin)
        T2 = _workspace(k, nimg, N * tiles_k(H, k), OW, Cin, dev)
        _transform("input_grad", k, Cg.data_ptr(), T2.data_ptr(), dx.data_ptr(), nimg, H, W, Cin, st)
    return dx


grad_spectra_k, input_grad_k = grad_spectra, input_grad


class ConvKxKFunction(torch.autograd.Function):
    """y = conv2d(x, bank) (k x k, stride 1, no padding, channels-last) as an FFT convolution with both gradients in the frequency
    domain (one transform of the output gradient's disjoint tiles serves both) -- `winograd.Conv5x5Function`'s FFT branch for
    the kernel sizes Winograd F(m, 5) does not cover."""

    @staticmethod
    def forward(ctx, x, bank):
        keep: list = []
        k = bank.shape[-1]
        y = conv_kxk(x, spectra_for_k(bank.detach()), k, None, False, keep_V=keep)
        ctx.save_for_backward(bank, *keep)
        return y

    @staticmethod
    def backward(ctx, dy):
        bank, V = ctx.saved_tensors
        k = bank.shape[-1]
        dy = dy.contiguous(memory_format=torch.channels_last)
        G = grad_spectra_k(dy, k)
        dx = input_grad_k(dy, bank, G) if ctx.needs_input_grad[0] else None
        dbank = filter_grad_k(V, dy, bank.shape[1], k, G).to(bank.dtype) if ctx.needs_input_grad[1] else None
        return dx, dbank
