"""The 16-multiple channel contractions of the FFT convolution (csrc/cgemm3m_c16.hip) on the device: the packed filter operand, the
forward-form contraction and the filter gradient's against fp64 with derived bounds, `ConvKxKFunction` / `conv5x5` on channel counts
that used to fall to the library's GEMM, and the steerable network whose hidden layers have 144 channels.

Bounds.  An fp32 sum of n products in any order is within gamma_n sum |product| of the exact one, gamma_n = n 2^-24 / (1 - n 2^-24).
The contraction computes, per output element, T1 = sum_k Ar Br, T2 = sum_k Ai Bi, T3 = sum_k fl(Ar + Ai) fl(Br + Bi) over the Cin input
channels and returns Cr = fl(T1 - T2), Ci = fl(fl(T3 - T1) - T2).  With m = sum_k (|Ar| + |Ai|)(|Br| + |Bi|):
  * T3's operands carry one rounding each (2 of the "+ 4"), the sum Cin roundings, the two combining subtractions one each (the other
    2): every one of T1, T2, T3 is within gamma_{Cin + 4} of its exact value times its own sum of magnitudes;
  * sum |Ar Br| + sum |Ai Bi| <= m and sum |Ar + Ai||Br + Bi| <= m, so Cr is within gamma_{Cin + 4} m, and Ci -- which carries all three
    sums, T3's magnitudes AND those of T1 + T2 -- within 2 gamma_{Cin + 4} m.
One bound for both parts: |err| <= 2 gamma_{Cin + 4} m.  The filter gradient's contraction is the same arithmetic with the M tiles as
the summation axis (P3 = sum_m fl(Vr - Vi) fl(Gr + Gi), Dr = fl(P1 + P2), Di = fl(fl(P1 - P2) - P3)): 2 gamma_{M + 4} sum_m (|Vr| + |Vi|)(|Gr| + |Gi|).
Convolutions and network steps follow the project's rule: each tensor relative to its own largest entry against the fp64 CPU result,
at most 4 x the error of the fp32 CPU plain-op path, which is computed here on the host that runs the test."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd import _lib
from equiadapt_amd.images.canonicalization_networks import fftconv
from equiadapt_amd.images.canonicalization_networks import steerable_networks as sn

pytestmark = pytest.mark.gpu

NF = fftconv.F
SENTINEL = -12345.0
GUARD = 64                      # floats in front of and behind a payload: keeps the 16-byte alignment


def _gamma(n: int) -> float:
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _guarded(numel: int, dev, fill=SENTINEL):
    """(whole buffer, payload view) with GUARD floats of `fill` on either side; the payload starts filled too."""
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf: torch.Tensor, fill=SENTINEL) -> bool:
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def _pitch(M: int) -> int:
    return _lib.load().eqa_fft48k5_tile_pitch(M)


def _spectra(M: int, C: int, dev, seed: int):
    """Random tile spectra in the layout of `spectra_buffer`, (F, pitch, 2C) rows [Re x 16 | Im x 16] per 16 channels, inside guards;
    the pitch's padding row (even M) is NaN: nothing may depend on it.  -> (guarded buffer, (F, M, 2C) view, Re, Im (F, M, C) fp64)."""
    pitch = _pitch(M)
    buf, flat = _guarded(NF * pitch * 2 * C, dev)
    g = torch.Generator().manual_seed(seed)
    full = flat.view(NF, pitch, 2 * C)
    full[:, :M] = torch.randn(NF, M, 2 * C, generator=g).to(dev)
    full[:, M:] = math.nan
    V = full[:, :M]
    ri = torch.empty(NF, M, 2 * C, dtype=torch.float64, device=dev)
    ri[:, :, fftconv._order(C, 16).to(dev)] = V.double()              # position p of a row holds [Re | Im][order[p]]
    return buf, V, ri[:, :, :C], ri[:, :, C:]


@functools.lru_cache(maxsize=None)
def _bank(cout: int, cin: int, k: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 * k + cin + cout)
    return torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)


def _real_form_parts(B: torch.Tensor, cin: int, cout: int):
    """Br, Bi (F, Cin, Cout) out of the library form (F, 2Cin, 2Cout): rows [Re x 16 | Im x 16] per 16 input channels, columns
    interleaved complex; the Re rows hold [Br | Bi]."""
    ci = torch.arange(cin, device=B.device)
    rows = B[:, (ci // 16) * 32 + ci % 16]
    return rows[:, :, 0::2], rows[:, :, 1::2]


# ---------------------------------------------------------------------------------------------------------------------------------
# the packed operand

@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("cout,cin", [(16, 16), (80, 48), (144, 144)])
def test_packed_operand(k, cout, cin, monkeypatch):
    """Br, Bi are the entries of the real form bit for bit (both signs of `correlate`), Bs = fl32(Br + Bi), pad columns exactly zero;
    the bank is unchanged; two launches give the same bits."""
    dev = torch.device("cuda:0")
    bank = _bank(cout, cin, k).to(dev)
    bank0 = bank.clone()
    for correlate in (True, False):
        monkeypatch.setattr(fftconv, "GEMM_C16", False)
        real = fftconv.spectra_for_k(bank, correlate)
        assert isinstance(real, torch.Tensor) and real.shape == (NF, 2 * cin, 2 * cout)
        monkeypatch.setattr(fftconv, "GEMM_C16", True)
        sp = fftconv.spectra_for_k(bank, correlate)
        assert isinstance(sp, fftconv.Spectra3MC16) and (sp.cin, sp.cout) == (cin, cout)
        assert sp.data.numel() == _lib.load().eqa_fft48_spectra3m_c16_floats(cin, cout)
        br, bi, bs = sp.unpack(pad=True)
        want_r, want_i = _real_form_parts(real, cin, cout)
        assert torch.equal(br[..., :cout], want_r) and torch.equal(bi[..., :cout], want_i)
        assert torch.equal(bs[..., :cout], br[..., :cout] + bi[..., :cout])
        for part in (br, bi, bs):
            assert not part[..., cout:].contiguous().view(torch.int32).any()       # +0.0, not -0.0
        assert torch.equal(fftconv.spectra_for_k(bank, correlate).data, sp.data)
    assert torch.equal(bank, bank0)


def test_packed_operand_inside_guards():
    """The C entry points write exactly eqa_fft48_spectra3m_c16_floats floats, every one of them."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    for k, cout, cin in [(5, 80, 48), (3, 16, 16)]:
        bank = _bank(cout, cin, k).to(dev)
        buf, b3 = _guarded(lib.eqa_fft48_spectra3m_c16_floats(cin, cout), dev, math.nan)
        if k == 5:
            st = lib.eqa_fft48k5_filter_spectra3m_c16(bank.data_ptr(), b3.data_ptr(), cout, cin, 1, _stream())
        else:
            st = lib.eqa_fft48_filter_spectra3m_c16(bank.data_ptr(), b3.data_ptr(), cout, cin, k, 1, _stream())
        assert st == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all()) and not torch.isnan(b3).any()
        assert torch.equal(b3, fftconv.filter_spectra3m_c16(bank).data)


# ---------------------------------------------------------------------------------------------------------------------------------
# the forward-form contraction

# (M, Cin, Cout): one row, one stage, half a column block; odd S, a second row tile of one row, 1 1/2 blocks; pitch 65 != M; three row
# tiles; the network's own counts (S = 9); 288
CONTRACT = [(1, 16, 16), (65, 48, 48), (64, 32, 80), (130, 80, 16), (33, 144, 144), (7, 288, 288)]


@pytest.mark.parametrize("M,cin,cout", CONTRACT)
def test_contraction_against_fp64(M, cin, cout):
    """Mo = V . B per frequency against the fp64 complex product of the de-grouped V with the unpacked Br, Bi:
    |err| <= 2 gamma_{Cin + 4} sum_k (|Ar| + |Ai|)(|Br| + |Bi|) per element, both parts (derivation: the module docstring).  Every payload
    element is written, the pitch's padding row and the guards keep the sentinel, V and B3 are unchanged, two launches give the
    same bits, and `contract` is this entry point."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    assert not lib.eqa_fft48k5_cgemm3m_supported(cin, cout)
    sp = fftconv.filter_spectra3m_c16(_bank(cout, cin, 3).to(dev))
    vbuf, V, ar, ai = _spectra(M, cin, dev, seed=M + cin)
    vbuf0, b30 = vbuf.clone(), sp.data.clone()
    br, bi, _ = (t.double() for t in sp.unpack())
    pitch = _pitch(M)

    def launch():
        mbuf, mo = _guarded(NF * pitch * 2 * cout, dev)
        assert lib.eqa_fft48_cgemm3m_c16(V.data_ptr(), sp.data.data_ptr(), mo.data_ptr(), M, cin, cout, _stream()) == 0
        torch.cuda.synchronize()
        return mbuf, mo.view(NF, pitch, 2 * cout)

    mbuf, mo = launch()
    assert _guards_intact(mbuf)
    assert not (mo[:, :M] == SENTINEL).any()
    assert (mo[:, M:] == SENTINEL).all()
    got = mo[:, :M].double()
    cr = torch.bmm(ar, br) - torch.bmm(ai, bi)
    ci = torch.bmm(ar, bi) + torch.bmm(ai, br)
    bound = 2.0 * _gamma(cin + 4) * torch.bmm(ar.abs() + ai.abs(), br.abs() + bi.abs())
    er, ei = (got[..., 0::2] - cr).abs(), (got[..., 1::2] - ci).abs()
    print(f"({M}, {cin}, {cout}): largest err / bound: Re {float((er / bound).max()):.3f}, Im {float((ei / bound).max()):.3f}")
    assert (er <= bound).all() and (ei <= bound).all()
    assert torch.equal(vbuf.view(torch.int32), vbuf0.view(torch.int32)) and torch.equal(sp.data, b30)
    _, mo2 = launch()
    assert torch.equal(mo2[:, :M], mo[:, :M])
    via = fftconv.contract(V, sp, M)
    assert fftconv.LAST_CONTRACTION == "c16" and torch.equal(via, mo[:, :M])


# ---------------------------------------------------------------------------------------------------------------------------------
# the filter gradient's contraction

# (M, Cin, Cout); at (48, 48): M at, just below and just above whole K-stages of 16 tiles (one and two)
WGRAD = [(1, 16, 16), (2, 16, 48), (17, 48, 16), (33, 144, 144), (16, 48, 48), (31, 48, 48), (32, 48, 48), (33, 48, 48)]


@pytest.mark.parametrize("M,cin,cout", WGRAD)
def test_filter_gradient_contraction_against_fp64(M, cin, cout):
    """D[f] = V[f]^T conj(G[f]) over the tiles, D3 (F, Cin, 2, Cout) = Dr | Di, against fp64:
    |err| <= 2 gamma_{M + 4} sum_m (|Vr| + |Vi|)(|Gr| + |Gi|).  D is fully written, guards intact, inputs unchanged, two launches the same bits."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    vbuf, V, vr, vi = _spectra(M, cin, dev, seed=3 * M + cin)
    gbuf, G, gr, gi = _spectra(M, cout, dev, seed=5 * M + cout + 1)
    vbuf0, gbuf0 = vbuf.clone(), gbuf.clone()

    def launch():
        dbuf, d = _guarded(NF * cin * 2 * cout, dev)
        assert lib.eqa_fft48_wgrad3m_c16(V.data_ptr(), G.data_ptr(), d.data_ptr(), M, cin, cout, _stream()) == 0
        torch.cuda.synchronize()
        return dbuf, d.view(NF, cin, 2, cout)

    dbuf, d = launch()
    assert _guards_intact(dbuf)
    assert not (d == SENTINEL).any()
    vrt, vit = vr.transpose(1, 2), vi.transpose(1, 2)
    dr = torch.bmm(vrt, gr) + torch.bmm(vit, gi)
    di = torch.bmm(vit, gr) - torch.bmm(vrt, gi)
    bound = 2.0 * _gamma(M + 4) * torch.bmm(vrt.abs() + vit.abs(), gr.abs() + gi.abs())
    er, ei = (d[:, :, 0].double() - dr).abs(), (d[:, :, 1].double() - di).abs()
    print(f"({M}, {cin}, {cout}): largest err / bound: Re {float((er / bound).max()):.3f}, Im {float((ei / bound).max()):.3f}")
    assert (er <= bound).all() and (ei <= bound).all()
    assert torch.equal(vbuf.view(torch.int32), vbuf0.view(torch.int32)) and torch.equal(gbuf.view(torch.int32), gbuf0.view(torch.int32))
    _, d2 = launch()
    assert torch.equal(d2, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# convolutions

def _rel(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def _conv_case(cout, cin, k):
    """x, bank, dy on the CPU; the fp64 output and gradients; per tensor 4 x the error of the fp32 CPU plain-op path.  Shared."""
    g = torch.Generator().manual_seed(7 * k + cin)
    x = torch.randn(2, cin, 20, 20, generator=g)
    bank = _bank(cout, cin, k)
    dy = torch.randn(2, cout, 21 - k, 21 - k, generator=g)
    res = {}
    for dt in (torch.float64, torch.float32):
        xx, bb = x.to(dt).clone().requires_grad_(True), bank.to(dt).clone().requires_grad_(True)      # (.to is the tensor itself in fp32)
        y = F.conv2d(xx, bb)
        y.backward(dy.to(dt))
        res[dt] = {"y": y.detach(), "dx": xx.grad, "dbank": bb.grad}
    ref = res[torch.float64]
    tol = {key: 4.0 * _rel(res[torch.float32][key], ref[key]) for key in ref}
    return x, bank, dy, ref, tol


@pytest.mark.parametrize("knob", [True, False])
@pytest.mark.parametrize("cout,cin,k", [(80, 48, 3), (80, 48, 5), (80, 48, 7), (144, 144, 7)])
def test_conv_function_routes_and_accuracy(cout, cin, k, knob, monkeypatch):
    """`ConvKxKFunction` on banks the existing kernels do not take: output and both gradients under the project's rule, both
    contractions on the new kernels -- and on the library's with GEMM_C16 off, under the same rule."""
    dev = torch.device("cuda:0")
    monkeypatch.setattr(fftconv, "GEMM_C16", knob)
    monkeypatch.setattr(fftconv, "LAST_CONTRACTION", None)
    monkeypatch.setattr(fftconv, "LAST_WGRAD", None)
    x, bank, dy, ref, tol = _conv_case(cout, cin, k)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = bank.to(dev).requires_grad_(True)
    y = fftconv.ConvKxKFunction.apply(xd, bd)
    y.backward(dy.to(dev))
    want = "c16" if knob else "lib"
    assert fftconv.LAST_CONTRACTION == want and fftconv.LAST_WGRAD == want
    errs = {"y": _rel(y, ref["y"]), "dx": _rel(xd.grad, ref["dx"]), "dbank": _rel(bd.grad, ref["dbank"])}
    print(f"({cout}, {cin}, {k}) {want}: " + ", ".join(f"{key} {errs[key]:.2e} / {tol[key]:.2e}" for key in errs))
    assert all(errs[key] <= tol[key] for key in errs), (errs, tol)


def test_conv5x5_family_takes_the_operand():
    """k = 5: `conv5x5` with bias / ReLU on both sides under the project's rule; a `GroupedMap` gives the same bits as the channels-last
    map; ``stats`` returns the same map; ``sums_k`` the window sums of the output (the project's rule against fp64)."""
    dev = torch.device("cuda:0")
    cout, cin = 80, 48
    x, bank, _, _, _ = _conv_case(cout, cin, 5)
    g = torch.Generator().manual_seed(5)
    ib, ob = torch.randn(cin, generator=g) * 0.3, torch.randn(cout, generator=g) * 0.3

    def plain(dt):
        y = torch.relu(F.conv2d(torch.relu(x.to(dt) + ib.to(dt)[None, :, None, None]), bank.to(dt)) + ob.to(dt)[None, :, None, None])
        sums = torch.stack([torch.stack([y[:, :, i:i + 12, j:j + 12].sum((2, 3)) for j in range(5)], -1) for i in range(5)], -2)
        return y, sums

    (y64, s64), (y32, s32) = plain(torch.float64), plain(torch.float32)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    sp = fftconv.spectra_for(bank.to(dev))
    assert isinstance(sp, fftconv.Spectra3MC16)
    y = fftconv.conv5x5(xd, sp, ob.to(dev), True, ib.to(dev), True)
    assert fftconv.LAST_CONTRACTION == "c16"
    assert _rel(y, y64) <= 4.0 * _rel(y32, y64)
    grouped = fftconv.GroupedMap(xd.permute(0, 2, 3, 1).reshape(2, 20, 20, cin // 16, 16).permute(0, 3, 1, 2, 4).contiguous())
    assert torch.equal(grouped.to_channels_last(), xd)
    assert torch.equal(fftconv.conv5x5(grouped, sp, ob.to(dev), True, ib.to(dev), True), y)
    sums = fftconv.conv5x5(xd, sp, ob.to(dev), True, ib.to(dev), True, sums_k=5)
    assert sums.shape == (2, cout, 5, 5) and sums.dtype == torch.float64
    assert _rel(sums, s64) <= 4.0 * _rel(s32, s64)
    if fftconv.output_stats_supported(2, 16, 16, cout):
        stats = []
        ys = fftconv.conv5x5(xd, sp, None, False, stats=stats)
        assert torch.equal(ys, fftconv.conv5x5(xd, sp, None, False)) and stats[0].shape[1:] == (cout, 2)


def test_headline_channel_counts_keep_their_kernel():
    """256 -> 256 still runs eqa_fft48k5_cgemm3m* in the form `gemm_form` names, and its filter gradient eqa_fft48k5_wgrad3m."""
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    x = torch.randn(1, 256, 48, 48, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bank = (torch.randn(256, 256, 5, 5, device=dev) / 80).requires_grad_(True)
    sp = fftconv.spectra_for(bank.detach())
    assert isinstance(sp, fftconv.Spectra3M)
    fftconv.conv5x5(x.detach(), sp, None, False)
    assert fftconv.LAST_CONTRACTION == "3m" and fftconv.LAST_FORM == fftconv.gemm_form(256, 256)
    del sp
    fftconv.ConvKxKFunction.apply(x, bank).sum().backward()
    assert fftconv.LAST_CONTRACTION == "3m" and fftconv.LAST_WGRAD == "3m"


# ---------------------------------------------------------------------------------------------------------------------------------
# the network

def _step(net, x, w):
    net.train()
    net.zero_grad()
    out = net(x)
    (out * w).sum().backward()
    return {"out": out.detach(), **{name: p.grad.detach().clone() for name, p in net.named_parameters()}}


def _errs(g, g64):
    errs = {}
    for key, r in g64.items():
        if float(r.abs().max()) == 0.0:
            errs[key] = 0.0 if float(g[key].abs().max()) == 0.0 else math.inf
        else:
            errs[key] = _rel(g[key], r)
    return errs


@functools.lru_cache(maxsize=None)
def _network_case():
    """The steerable network with 16 fields (144 hidden channels), k = 7, 3 layers on 64 x 64: hidden maps of 58 x 58 = 8 tiles for a
    batch of two.  Norm parameters and running statistics off their initial values; eval forward and one training step on the fp64 and
    fp32 CPU plain-op paths.  Shared."""
    in_shape = (3, 64, 64)
    torch.manual_seed(0)
    net = ea.ESCNNSteerableNetwork(in_shape, 16, 7, "rotation", 3)
    with torch.no_grad():
        net.train()
        net(torch.randn(2, *in_shape))
        for m in net.block:
            if isinstance(m, sn.FieldNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, *in_shape)
    w = torch.tensor([[[0.7, -1.1], [0.4, 0.9]], [[-0.6, 0.8], [1.2, -0.3]]])
    n64, n32 = copy.deepcopy(net).double(), copy.deepcopy(net)
    with torch.no_grad():
        e64, e32 = n64.eval()(x.double()), n32.eval()(x)
    g64, g32 = _step(n64, x.double(), w.double()), _step(n32, x, w)
    return net, x, w, e64, 4.0 * _rel(e32, e64), g64, 4.0 * max(_errs(g32, g64).values())


def test_network_hidden_layers_run_the_contraction(monkeypatch):
    """One eval forward and one training step: the routes, the contraction that ran, and the project's rule for the output and every
    parameter gradient against the fp64 CPU network."""
    dev = torch.device("cuda:0")
    for name in ("EQA_STEER_LIFT_KERNEL", "EQA_FIELD_NORM_KERNEL", "EQA_FOURIER_KERNEL"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(fftconv, "GEMM_C16", True)
    net, x, w, e64, etol, g64, gtol = _network_case()
    dnet = copy.deepcopy(net).to(dev)
    xd, wd = x.to(dev), w.to(dev)
    monkeypatch.setattr(fftconv, "LAST_CONTRACTION", None)
    with torch.no_grad():
        out = dnet.eval()(xd)
    err = _rel(out, e64)
    print(f"eval tolerance {etol:.2e}, device rel err {err:.2e}; routes {dnet.last_routes}")
    assert dnet.last_routes == ["steer_lift", "fft", "fft", "window_sums"]
    assert fftconv.LAST_CONTRACTION == "c16"
    assert err <= etol
    monkeypatch.setattr(fftconv, "LAST_CONTRACTION", None)
    monkeypatch.setattr(fftconv, "LAST_WGRAD", None)
    g = _step(dnet, xd, wd)
    errs = _errs(g, g64)
    print(f"step tolerance {gtol:.2e}, device largest rel err {max(errs.values()):.2e}; routes {dnet.last_routes}")
    assert dnet.last_routes == ["steer_lift", "fft", "fft", "window_sums"]
    assert fftconv.LAST_CONTRACTION == "c16" and fftconv.LAST_WGRAD == "c16"
    assert set(g) == set(g64) and max(errs.values()) <= gtol, errs
