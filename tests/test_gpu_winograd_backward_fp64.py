"""GPU: the backward side of the Winograd 5x5 convolution (csrc/winograd.hip, images/canonicalization_networks/winograd.py)
against fp64 references, each kernel and each step of the Python route on its own, then ``Conv5x5Function`` end to end.

Cases, references, measures and budgets: tests/winograd_backward_cases.py (CPU only; tests/test_winograd_fp64_reference.py
checks them and plants errors).  Every test switches the FFT convolution's training forward off, so that the Winograd branch of
``Conv5x5Function`` is the one under test, and passes the tile size m explicitly; every case runs m = 2 and m = 4.

    (i)   eqa_winograd_f{m}k5_output_adjoint on dy             dM = A dY A^T          a-priori bound 64 u |A| |dY| |A|^T
    (ii)  eqa_winograd_f{m}k5_input_padded (pad = 4) on dy     V = B^T pad(dy) B      a-priori bound 64 u |B^T| |d| |B|
          eqa_winograd_f{m}k5_input on x (the filter gradient's V; the plain form of the strip walk)   the same bound
    (iii) winograd.filter_grad, folded back with G in fp64     d_bank                 budget "d_bank"
    (iv)  winograd.conv5x5(dy, U_t, pad = 4)                   d_x                    budgets "d_x:interior", "d_x:border"
    (v)   Conv5x5Function.apply(x, bank, m) and .backward()    y within 2e-5, both gradients under the same budgets

A budget is 4 times the error of torch's fp32 CPU evaluation of the same chain against fp64 autograd, pooled over the cases
and computed at run time (d_bank 6.9e-5, d_x 4.2e-5 / 3.9e-5 where this was written); nothing is taken from the kernels.

What the cases reach (``launch_plan`` restates the host code's strip arithmetic; the CPU test asserts these figures):
  off-32         32 -> 48 at 12 x 16: the library's strided-batched GEMM both ways (48 is off the 32-multiples), non-square, one
                 strip per tile row (two even ones in the padded m = 2 form), work counts off the multiples of 8
  strips         32 -> 32 at 32 x 40: m = 4 plain TX = 9, strips (5, 4); its dy is 28 x 36, so the padded form has TX = 10 (m = 4,
                 strips (5, 5), 48 work items) and TX = 20 (m = 2, five strips of 4, 240 work items): even strips, multiples of 8
  strips-padded  32 -> 32 at 36 x 44, dy 32 x 40: padded m = 4 TX = 11, strips (6, 5), 54 work items; padded m = 2 TX = 22, strips
                 5, 5, 5, 5, 2, 270 work items; plain m = 4 TX = 10 (5, 5), plain m = 2 TX = 20
  wide           288 -> 320 at 12 x 12: blockIdx.y = 1 with 32 (x) or 64 (dy) of 256 lanes in every kernel
  chunks         9 images, 32 -> 64 at 12 x 12 with winograd.CHUNK_IMAGES = 2: five chunks (2, 2, 2, 2, 1) for m = 2, (8, 1) for
                 m = 4, V recomputed per chunk; and with the default chunk, KEEP_V_FOR_BACKWARD True and False

Measured on an MI355X (profiles/r15/winograd_backward_fp64.txt lists every case; findings in profiles/r15/README.md), kernel
error / fp32 CPU error: the three transforms 0.65 - 1.04 (3 - 5 % of the a-priori bound), d_bank 0.42 - 2.77, d_x interior
0.75 - 1.88, border 0.77 - 1.59, forward 0.68 - 1.83 (at most 1.5e-5 of the 2e-5).  The bound is 4.  d_bank's 2.77 (960 tiles,
m = 2) is the order and length of the fp32 sum over tiles in the library GEMM, not a kernel: a one-by-one fp32 sum of the same
products on the CPU is 1.6 x the CPU GEMM's error, and splitting the sum into chunks brings the ratio from 1.21 to 0.42.

Every figure is printed as reference (fp32 CPU) error, kernel error and their ratio; with EQA_WINOGRAD_FP64_LOG=<file> it is
appended to that file as well.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import winograd_backward_cases as wc  # noqa: E402

RUNS = [(c.name, m) for c in wc.CASES for m in wc.tiles_of(c)]
IDS = [f"{n}-m{m}" for n, m in RUNS]
# how winograd.py walks the batch: (name, CHUNK_IMAGES or None for the default, KEEP_V_FOR_BACKWARD)
MODES = {"default": (None, True), "chunk2": (2, True), "no-keep-v": (None, False)}


def modes_of(name):
    return ("chunk2", "default", "no-keep-v") if name == "chunks" else ("default",)


MODE_RUNS = [(n, m, mode) for n, m in RUNS for mode in modes_of(n)]
MODE_IDS = [f"{n}-m{m}-{mode}" for n, m, mode in MODE_RUNS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def winograd_branch(monkeypatch):
    from equiadapt_amd.images.canonicalization_networks import fftconv

    monkeypatch.setattr(fftconv, "TRAIN_FORWARD", False)


def _set_mode(monkeypatch, mode):
    from equiadapt_amd.images.canonicalization_networks import winograd

    chunk, keep = MODES[mode]
    if chunk is not None:
        monkeypatch.setattr(winograd, "CHUNK_IMAGES", chunk)
    monkeypatch.setattr(winograd, "KEEP_V_FOR_BACKWARD", keep)
    return winograd.CHUNK_IMAGES


def _nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def _record(quantity, name, m, what, ref_err, got_err, bound):
    """Print the figure (shown when the assertion below it fails) and append it to the log file if one is asked for."""
    ratio = got_err / ref_err if ref_err > 0 else (0.0 if got_err == 0 else float("inf"))
    line = (f"{quantity:13s} {name:14s} m={m} {what:34s} fp32-cpu {ref_err:9.3e}  kernel {got_err:9.3e}  ratio {ratio:7.3f}  "
            f"bound {bound:9.3e}")
    print(line)
    path = os.environ.get("EQA_WINOGRAD_FP64_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _transform(dev, fn_name, src, m, pad=None):
    """One direct call of a transform entry point on a channels-last map; returns the (tiles, P, C) result."""
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    B, C, H, W = src.shape
    n = m + 4
    if fn_name == "output_adjoint":
        tiles = B * (H // m) * (W // m)
    else:
        p = pad or 0
        tiles = B * ((H + 2 * p - 4) // m) * ((W + 2 * p - 4) // m)
    d = _nhwc(src, dev)
    out = torch.empty((tiles, n * n, C), dtype=torch.float32, device=dev)
    fn = getattr(lib, f"eqa_winograd_f{m}k5_{fn_name}")
    with torch.cuda.device(dev):
        if fn_name == "output_adjoint":
            st = fn(d.data_ptr(), out.data_ptr(), B, H, W, C, ops._stream())
        elif fn_name == "input_padded":
            st = fn(d.data_ptr(), out.data_ptr(), B, H, W, C, pad, ops._stream())
        else:
            st = fn(d.data_ptr(), out.data_ptr(), None, 0, B, H, W, C, ops._stream())
    assert st == 0, (fn_name, st)
    return out


def _check_transform(quantity, name, m, got, ref, cpu32):
    err = wc.measure_transform(got, ref)
    _record(quantity, name, m, "share of the a-priori bound", wc.measure_transform(cpu32, ref), err, 1.0)
    assert err <= 1.0, (quantity, name, m, err)


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_output_adjoint_matches_fp64(dev, name, m):
    """(i) dM = A dY A^T, eqa_winograd_f{m}k5_output_adjoint called directly."""
    dy = wc.inputs(name)[2]
    got = _transform(dev, "output_adjoint", dy, m)
    _check_transform("adjoint", name, m, got, wc.adjoint_reference(name, m), wc.output_adjoint(dy, m))


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_padded_input_transform_matches_fp64(dev, name, m):
    """(ii) V = B^T d B of dy zero-padded by 4 inside eqa_winograd_f{m}k5_input_padded: the clamped loads, the strip walk's
    sliding window and prefetch, the XCD work order."""
    dy = wc.inputs(name)[2]
    got = _transform(dev, "input_padded", dy, m, pad=4)
    _check_transform("input_padded", name, m, got, wc.padded_input_reference(name, m), wc.input_transform(dy, m, 4))


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_plain_input_transform_matches_fp64(dev, name, m):
    """The V that the filter gradient contracts: eqa_winograd_f{m}k5_input on x, the plain form of the same strip walk."""
    x = wc.inputs(name)[0]
    got = _transform(dev, "input", x, m)
    _check_transform("input", name, m, got, wc.plain_input_reference(name, m), wc.input_transform(x, m))


@pytest.mark.parametrize("name,m,mode", MODE_RUNS, ids=MODE_IDS)
def test_filter_gradient_matches_fp64(dev, monkeypatch, name, m, mode):
    """(iii) winograd.filter_grad (input transform, output adjoint, one accumulating product per plane and chunk), folded back
    with G in fp64 as Conv5x5Function.backward does."""
    from equiadapt_amd.images.canonicalization_networks import winograd

    c = wc.CASE_BY_NAME[name]
    chunk_images = _set_mode(monkeypatch, mode)
    if mode == "chunk2":
        assert wc.chunk_sizes(c.B, m, chunk_images) == ((2, 2, 2, 2, 1) if m == 2 else (8, 1))
    x, _, dy = wc.inputs(name)
    dU = winograd.filter_grad(_nhwc(x, dev), _nhwc(dy, dev), m)
    assert dU.shape == ((m + 4) ** 2, c.Cin, c.Cout)
    err = wc.measure(wc.fold_back(dU.cpu(), m, torch.float32), wc.reference(name).d_bank)
    _record("d_bank", name, m, f"filter_grad, {mode}", wc.cpu_chain_errors()[("d_bank", name, m)], err, wc.budgets()["d_bank"])
    assert err <= wc.budgets()["d_bank"], (name, m, mode, err, wc.budgets()["d_bank"])


def _check_input_gradient(got, name, m, what):
    errs = wc.measure_input_gradient(got, wc.reference(name).d_x)
    for q, v in errs.items():
        _record(q, name, m, what, wc.cpu_chain_errors()[(q, name, m)], v, wc.budgets()[q])
    for q, v in errs.items():
        assert v <= wc.budgets()[q], (name, m, what, q, v, wc.budgets()[q])


@pytest.mark.parametrize("name,m,mode", MODE_RUNS, ids=MODE_IDS)
def test_input_gradient_matches_fp64(dev, monkeypatch, name, m, mode):
    """(iv) d_x = conv5x5(dy zero-padded by 4, flipped and transposed bank): the padded input transform, the plane products with
    Cin and Cout exchanged (which swaps the GEMM route where one of them is off the 32-multiples), the output transform."""
    from equiadapt_amd.images.canonicalization_networks import winograd

    c = wc.CASE_BY_NAME[name]
    _set_mode(monkeypatch, mode)
    _, bank, dy = wc.inputs(name)
    bank_t = bank.to(dev).flip(-1, -2).transpose(0, 1).contiguous()
    got = winograd.conv5x5(_nhwc(dy, dev), winograd.transform_filters(bank_t, m), None, False, pad=4)
    assert got.shape == (c.B, c.Cin, c.H, c.W)
    _check_input_gradient(got, name, m, f"conv5x5(pad=4), {mode}")


@pytest.mark.parametrize("name,m,mode", MODE_RUNS, ids=MODE_IDS)
def test_conv5x5_function_matches_fp64(dev, monkeypatch, name, m, mode):
    """(v) Conv5x5Function end to end: the forward within the 2e-5 of test_winograd_conv_matches_direct, both gradients under
    the budgets of (iii) and (iv).  With one chunk and KEEP_V_FOR_BACKWARD the filter gradient contracts the forward's V."""
    from equiadapt_amd.images.canonicalization_networks import winograd

    c = wc.CASE_BY_NAME[name]
    _set_mode(monkeypatch, mode)
    x, bank, dy = wc.inputs(name)
    xd = _nhwc(x, dev).requires_grad_(True)
    bd = bank.to(dev).requires_grad_(True)
    y = winograd.Conv5x5Function.apply(xd, bd, m)
    assert y.shape == (c.B, c.Cout, c.H - 4, c.W - 4)
    y.backward(dy.to(dev))
    want = wc.reference(name)
    e_y = wc.measure(y, want.y)
    e_b = wc.measure(bd.grad, want.d_bank)
    _record("forward", name, m, f"Conv5x5Function, {mode}", wc.cpu_chain_errors()[("forward", name, m)], e_y, wc.FORWARD_BOUND)
    _record("d_bank", name, m, f"Conv5x5Function, {mode}", wc.cpu_chain_errors()[("d_bank", name, m)], e_b, wc.budgets()["d_bank"])
    assert xd.grad.shape == x.shape and bd.grad.shape == bank.shape
    _check_input_gradient(xd.grad, name, m, f"Conv5x5Function, {mode}")
    assert e_y <= wc.FORWARD_BOUND, (name, m, mode, e_y)
    assert e_b <= wc.budgets()["d_bank"], (name, m, mode, e_b, wc.budgets()["d_bank"])


@pytest.mark.parametrize("m", wc.TILES)
def test_entry_point_contract(dev, m):
    """nimg = 0 is EQA_OK and writes nothing; a logical size that m does not divide is -3 (unsupported) before any launch."""
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    n = m + 4
    C, H, W = 32, 12, 16
    d = torch.randn(1, C, H, W, device=dev).contiguous(memory_format=torch.channels_last)
    sentinel = 1234.5
    adj, pad = (getattr(lib, f"eqa_winograd_f{m}k5_{k}") for k in ("output_adjoint", "input_padded"))
    with torch.cuda.device(dev):
        st = ops._stream()
        out = torch.full((1 * (H // m) * (W // m) * n * n * C,), sentinel, dtype=torch.float32, device=dev)
        assert adj(d.data_ptr(), out.data_ptr(), 0, H, W, C, st) == 0
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
        out = torch.full((1 * ((H + 4) // m) * ((W + 4) // m) * n * n * C,), sentinel, dtype=torch.float32, device=dev)
        assert pad(d.data_ptr(), out.data_ptr(), 0, H, W, C, 4, st) == 0
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
        # H + 1 / W + 2 rows: never launched, the buffers are not touched
        for h, w in ((H + 1, W), (H, W + m // 2), (H + m - 1, W + 1)):
            assert h % m or w % m
            assert adj(d.data_ptr(), out.data_ptr(), 1, h, w, C, st) == -3, (h, w)
            assert pad(d.data_ptr(), out.data_ptr(), 1, h, w, C, 4, st) == -3, (h, w)
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
