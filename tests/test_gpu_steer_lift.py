"""The steerable lifting kernels (csrc/steer_lift.hip) on the device: forward, epilogue statistics and filter gradient against fp64
with derived bounds, `SteerLiftFunction`, the route inside ESCNNSteerableNetwork, and the refusals in front of every launch.

Bounds.  An fp32 sum of n products in any order (an fma chain included; zero terms add nothing) is within
gamma_n sum |product| of the exact one, gamma_n = n 2^-24 / (1 - n 2^-24).  The statistics are fp64 sums of exact terms: within
n 2^-52 sum |term| (n = pixels).  Network steps follow the project's rule: each tensor relative to its own largest entry against the
fp64 CPU step, at most 4 x the error of the fp32 CPU plain-op path; a reference that is exactly zero is met exactly."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import equiadapt_amd as ea
from equiadapt_amd import _lib, ops
from equiadapt_amd.images.canonicalization_networks import steerable_networks as sn

pytestmark = pytest.mark.gpu

# (Cin, K, fields, B, H, W): one output pixel, less than one 16-block; the layer of the test network (2 1/4 blocks); the
# configuration's 144 channels, one pixel past a 32-tile; one output row, R = 243; rows of exactly 32; the field limit, 16-pixel
# rows; five images of a single 31-pixel row (the tile walk crosses images at every step)
SHAPES = [(1, 5, 1, 1, 5, 5), (3, 7, 4, 2, 33, 33), (3, 7, 16, 2, 13, 39), (3, 9, 5, 1, 9, 41), (1, 9, 16, 3, 12, 40),
          (3, 5, 64, 1, 8, 20), (1, 7, 3, 5, 7, 37)]
SENTINEL = -12345.0
GUARD = 64                      # floats (fp32 buffers) or doubles in front of and behind a payload: keeps the 16-byte line


def _gamma(n: int) -> float:
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _guarded(numel: int, dtype, dev, fill=SENTINEL):
    """(whole buffer, payload view) with GUARD elements of `fill` on either side; the payload starts filled too."""
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf: torch.Tensor, fill=SENTINEL) -> bool:
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


@functools.lru_cache(maxsize=None)
def _case(shape):
    """x, bank, dy (fp32, CPU; x and dy channels-last) and the fp64 results with their magnitudes.  Shared, never modified."""
    cin, k, fields, B, H, W = shape
    g = torch.Generator().manual_seed(1000 * k + 10 * fields + cin)
    R = cin * k * k
    x = torch.randn(B, cin, H, W, generator=g).contiguous(memory_format=torch.channels_last)
    bank = torch.randn(9 * fields, cin, k, k, generator=g) / math.sqrt(R)
    dy = torch.randn(B, 9 * fields, H - k + 1, W - k + 1, generator=g).contiguous(memory_format=torch.channels_last)
    y64 = F.conv2d(x.double(), bank.double())
    ymag = F.conv2d(x.double().abs(), bank.double().abs())
    dw64 = torch.nn.grad.conv2d_weight(x.double(), bank.shape, dy.double())
    dwmag = torch.nn.grad.conv2d_weight(x.double().abs(), bank.shape, dy.double().abs())
    return x, bank, dy, y64, ymag, dw64, dwmag


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """The channels-last memory of t as a flat tensor."""
    return t.permute(0, 2, 3, 1).reshape(-1)


def _launch_fwd(shape, xd, wpk, with_part, dev):
    cin, k, fields, B, H, W = shape
    lib = _lib.load()
    n = B * (H - k + 1) * (W - k + 1) * 9 * fields
    ybuf, y = _guarded(n, torch.float32, dev)
    rows = lib.eqa_steer_lift_stat_rows(fields)
    assert rows >= 1
    pbuf, part = _guarded(rows * 9 * fields * 2, torch.float64, dev, math.nan) if with_part else (None, None)
    st = lib.eqa_steer_lift_fwd(xd.data_ptr(), wpk.data_ptr(), y.data_ptr(), part.data_ptr() if with_part else None, B, H, W, cin, k,
                                fields, _stream())
    assert st == 0
    torch.cuda.synchronize()
    return ybuf, y, pbuf, part


def _fp64_sums(y: torch.Tensor, fields: int):
    """(sums, magnitudes) (fields, 6) of a (B, 9 fields, H, W) map in fp64 torch ops."""
    ys = y.double().unflatten(1, (fields, 9))
    a0 = ys[:, :, 0]
    sq = (ys[:, :, 1:] ** 2).unflatten(2, (4, 2)).sum(dim=(0, 3, 4, 5))
    sums = torch.cat([a0.sum(dim=(0, 2, 3))[:, None], (a0 * a0).sum(dim=(0, 2, 3))[:, None], sq], dim=1)
    mags = torch.cat([a0.abs().sum(dim=(0, 2, 3))[:, None], (a0 * a0).sum(dim=(0, 2, 3))[:, None], sq], dim=1)
    return sums, mags


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_against_fp64(shape):
    """|y - conv2d_64(x, w)| <= gamma_R conv2d_64(|x|, |w|) per element, through the C entry into a guarded buffer: the guards are
    intact, no payload element is left unwritten, x and wpk are unchanged, two launches give the same bits."""
    dev = torch.device("cuda:0")
    cin, k, fields, B, H, W = shape
    x, bank, _, y64, ymag, _, _ = _case(shape)
    xd, wpk = x.to(dev), ops.pack_steer_lift_weights(bank.to(dev))
    wpk0 = wpk.clone()
    ybuf, y, _, _ = _launch_fwd(shape, xd, wpk, False, dev)
    assert _guards_intact(ybuf)
    assert not (y == SENTINEL).any()
    got = y.cpu().double()
    err = (got - _nhwc(y64)).abs()
    bound = _gamma(cin * k * k) * _nhwc(ymag)
    print(f"{shape}: largest err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(xd.cpu(), x) and torch.equal(wpk, wpk0)
    _, y2, _, _ = _launch_fwd(shape, xd, wpk, False, dev)
    assert torch.equal(y, y2)
    yw, none = ops.steer_lift(xd, wpk, k, fields)
    assert none is None and yw.shape == y64.shape and yw.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(_nhwc(yw), y)


@pytest.mark.parametrize("shape", SHAPES)
def test_statistics(shape):
    """part, pre-filled with NaN: every row written; the folded (fields, 6) sums within n 2^-52 sum |term| of fp64 torch sums of
    the returned y; `field_norm_scale_shift` of them equals that of `ops.field_norm_stats(y).sum(0)`; y is the same bits with and
    without part; two launches: the same bits."""
    dev = torch.device("cuda:0")
    cin, k, fields, B, H, W = shape
    x, bank, _, y64, _, _, _ = _case(shape)
    xd, wpk = x.to(dev), ops.pack_steer_lift_weights(bank.to(dev))
    _, y_plain, _, _ = _launch_fwd(shape, xd, wpk, False, dev)
    ybuf, y, pbuf, part = _launch_fwd(shape, xd, wpk, True, dev)
    assert _guards_intact(ybuf) and bool(torch.isnan(pbuf[:GUARD]).all() and torch.isnan(pbuf[-GUARD:]).all())
    assert not torch.isnan(part).any()
    assert torch.equal(y, y_plain)
    _, _, _, part2 = _launch_fwd(shape, xd, wpk, True, dev)
    assert torch.equal(part, part2)
    yw, sums = ops.steer_lift(xd, wpk, k, fields, with_stats=True)
    assert torch.equal(_nhwc(yw), y) and sums.shape == (fields, 6) and sums.dtype == torch.float64
    ch = part.view(-1, fields, 9, 2).sum(0)
    torch.testing.assert_close(sums, torch.cat([ch[:, 0, :], ch[:, 1:, 1].reshape(fields, 4, 2).sum(2)], dim=1), rtol=1e-13, atol=0.0)
    npix = B * (H - k + 1) * (W - k + 1)
    ref, mags = _fp64_sums(yw.cpu(), fields)
    err = (sums.cpu() - ref).abs()
    bound = npix * 2.0 ** -52 * mags
    print(f"{shape}: rows {part.numel() // (18 * fields)}, largest err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    weight, bias = torch.ones(fields, 5, device=dev), torch.zeros(fields, device=dev)
    mean, var, _, _ = sn.field_norm_scale_shift(sums, npix, weight, bias, 1e-5)
    mean2, var2, _, _ = sn.field_norm_scale_shift(ops.field_norm_stats(yw).sum(0), npix, weight, bias, 1e-5)
    torch.testing.assert_close(mean, mean2, rtol=1e-12, atol=0.0)
    torch.testing.assert_close(var, var2, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("shape", SHAPES)
def test_filter_gradient(shape):
    """|dbank - conv2d_weight_64(x, dy)| <= gamma_n conv2d_weight_64(|x|, |dy|), n = B OH OW; two launches: the same bits; dbank and
    the workspace sit in guarded buffers whose guards stay intact."""
    dev = torch.device("cuda:0")
    cin, k, fields, B, H, W = shape
    x, bank, dy, _, _, dw64, dwmag = _case(shape)
    lib = _lib.load()
    xd, dyd = x.to(dev), dy.to(dev)
    wsbytes = lib.eqa_steer_lift_wgrad_workspace_bytes(cin, k, fields)
    assert wsbytes > 0 and wsbytes % 4 == 0
    results = []
    for _ in range(2):
        wbuf, ws = _guarded(wsbytes // 4, torch.float32, dev)
        dbuf, db = _guarded(bank.numel(), torch.float32, dev)
        st = lib.eqa_steer_lift_wgrad(xd.data_ptr(), dyd.data_ptr(), ws.data_ptr(), db.data_ptr(), B, H, W, cin, k, fields, _stream())
        assert st == 0
        torch.cuda.synchronize()
        assert _guards_intact(wbuf) and _guards_intact(dbuf)
        results.append(db.clone())
    assert torch.equal(results[0], results[1])
    n = B * (H - k + 1) * (W - k + 1)
    err = (results[0].cpu().double().view_as(dw64) - dw64).abs()
    bound = _gamma(n) * dwmag
    print(f"{shape}: n {n}, largest err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(xd.cpu(), x) and torch.equal(dyd.cpu(), dy)
    assert torch.equal(ops.steer_lift_wgrad(xd, dyd, k).flatten(), results[0])


def _rel(a: torch.Tensor, ref: torch.Tensor) -> float:
    return float((a.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def test_function_gradients_and_no_grad():
    """SteerLiftFunction on the test network's layer with x.requires_grad: dx against the fp64 conv2d_input (4 x the fp32 CPU error),
    dbank within the filter gradient's bound; under no_grad no graph is kept."""
    dev = torch.device("cuda:0")
    shape = (3, 7, 4, 2, 33, 33)
    cin, k, fields, B, H, W = shape
    x, bank, dy, _, _, dw64, dwmag = _case(shape)
    dx64 = torch.nn.grad.conv2d_input(x.shape, bank.double(), dy.double())
    tol = 4.0 * _rel(torch.nn.grad.conv2d_input(x.shape, bank, dy), dx64)
    xd, bd = x.to(dev).requires_grad_(True), bank.to(dev).requires_grad_(True)
    y, sums = sn.SteerLiftFunction.apply(xd, bd, True)
    assert y.requires_grad and not sums.requires_grad
    y.backward(dy.to(dev))
    err = _rel(xd.grad, dx64)
    print(f"dx: tolerance {tol:.2e}, device rel err {err:.2e}")
    assert err <= tol
    n = B * (H - k + 1) * (W - k + 1)
    assert ((bd.grad.cpu().double() - dw64).abs() <= _gamma(n) * dwmag).all()
    with torch.no_grad():
        y2 = sn.SteerLiftFunction.apply(xd, bd)
    assert y2.grad_fn is None and not y2.requires_grad and torch.equal(y2, y)


# ---------------------------------------------------------------------------------------------------------------------------------
# the network

NETS = [((3, 33, 33), 4, 7, 2), ((1, 28, 28), 2, 5, 1)]


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
def _network_case(spec):
    """The network with norm parameters and running statistics that are not the initial ones, a batch of two, and on the fp64 / fp32
    CPU plain-op paths: its eval forward, then one training step (and the running statistics after it).  Shared."""
    in_shape, fields, k, layers = spec
    torch.manual_seed(0)
    net = ea.ESCNNSteerableNetwork(in_shape, fields, k, "rotation", layers)
    with torch.no_grad():
        net.train()
        net(torch.randn(4, *in_shape))
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
    running = {key: v.clone() for key, v in n64.named_buffers() if "running" in key}
    return net, x, w, e64, 4.0 * _rel(e32, e64), g64, 4.0 * max(_errs(g32, g64).values()), running


@pytest.mark.parametrize("spec", NETS)
@pytest.mark.parametrize("knob", [None, "0"])
def test_network_routes_and_accuracy(spec, knob, monkeypatch):
    """Eval forward and one training step with EQA_STEER_LIFT_KERNEL unset / "0": the tolerance rule against the fp64 CPU network,
    the launches `ops.KernelTimer` saw, `last_routes`, and the running statistics after the step."""
    dev = torch.device("cuda:0")
    layers = spec[3]
    net, x, w, e64, etol, g64, gtol, running = _network_case(spec)
    if knob is None:
        monkeypatch.delenv("EQA_STEER_LIFT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("EQA_STEER_LIFT_KERNEL", knob)
    monkeypatch.delenv("EQA_FIELD_NORM_KERNEL", raising=False)
    monkeypatch.delenv("EQA_FOURIER_KERNEL", raising=False)
    on = knob is None
    dnet = copy.deepcopy(net).to(dev)
    xd, wd = x.to(dev), w.to(dev)
    with torch.no_grad(), ops.KernelTimer() as t:
        out = dnet.eval()(xd)
    names = t.summary()
    err = _rel(out, e64)
    print(f"{spec} knob {knob}: eval tolerance {etol:.2e}, device rel err {err:.2e}; routes {dnet.last_routes}")
    assert err <= etol
    assert ("steer_lift" in names) == on and "steer_lift_wgrad" not in names and "field_norm_stats" not in names
    assert dnet.last_routes[0] == ("steer_lift" if on else "lib") and len(dnet.last_routes) == layers + 1
    with ops.KernelTimer() as t:
        g = _step(dnet, xd, wd)
    names = t.summary()
    errs = _errs(g, g64)
    print(f"{spec} knob {knob}: step tolerance {gtol:.2e}, device largest rel err {max(errs.values()):.2e}; routes {dnet.last_routes}")
    assert set(g) == set(g64) and max(errs.values()) <= gtol, errs
    stats_launches = names["field_norm_stats"][0] if "field_norm_stats" in names else 0
    if on:
        assert names["steer_lift"][0] == 1 and names["steer_lift_wgrad"][0] == 1 and stats_launches == layers - 1
    else:
        assert "steer_lift" not in names and "steer_lift_wgrad" not in names and stats_launches == layers
    assert dnet.last_routes[0] == ("steer_lift" if on else "lib")
    buffers = dict(dnet.named_buffers())
    for key, v in running.items():
        torch.testing.assert_close(buffers[key].cpu().double(), v, rtol=1e-4, atol=1e-5)


def test_cached_pack_goes_stale(monkeypatch):
    """In eval the packed weights are cached on the layer; an in-place change of conv.weights (a version bump) changes the output,
    to what a fresh copy of the changed network gives."""
    monkeypatch.delenv("EQA_STEER_LIFT_KERNEL", raising=False)
    dev = torch.device("cuda:0")
    net, x = _network_case(NETS[0])[:2]
    dnet = copy.deepcopy(net).to(dev).eval()
    xd = x.to(dev)
    with torch.no_grad():
        out1 = dnet(xd)
        assert "steer_lift" in dnet.block[0]._cache and torch.equal(dnet(xd), out1)
        dnet.block[0].weights.mul_(1.5)
        out2 = dnet(xd)
        fresh = copy.deepcopy(dnet)
        fresh.block[0]._cache.clear()
        assert not torch.equal(out1, out2) and torch.equal(out2, fresh(xd))


def test_entry_points_refuse_before_they_launch():
    """Shapes outside the predicate and maps smaller than the filter: unsupported, from NULL pointers too; NULL pointers and a negative
    batch: invalid; y / dy off the 16-byte line: unsupported; an empty batch: OK.  None of these launches anything."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = _stream()
    for cin, k, fields, H in ((2, 7, 4, 33), (3, 4, 4, 33), (3, 11, 4, 33), (3, 7, 0, 33), (3, 7, 65, 33), (3, 7, 4, 6)):
        assert lib.eqa_steer_lift_fwd(None, None, None, None, 2, H, 33, cin, k, fields, st) == -3
        assert lib.eqa_steer_lift_wgrad(None, None, None, None, 2, H, 33, cin, k, fields, st) == -3
    B, H, W, cin, k, fields = 2, 13, 13, 3, 7, 4
    x = torch.full((B, cin, H, W), 5.0, device=dev).contiguous(memory_format=torch.channels_last)
    wpk = torch.full((lib.eqa_steer_lift_packed_floats(cin, k, fields),), 5.0, device=dev)
    y = torch.full((B * 49 * 36 + 4,), 5.0, device=dev)
    part = torch.full((lib.eqa_steer_lift_stat_rows(fields), 36, 2), 5.0, dtype=torch.float64, device=dev)
    ws = torch.full((lib.eqa_steer_lift_wgrad_workspace_bytes(cin, k, fields) // 4,), 5.0, device=dev)
    dbank = torch.full((36, cin, k, k), 5.0, device=dev)
    px, pw, py, pp, ps, pd = (t.data_ptr() for t in (x, wpk, y, part, ws, dbank))
    args = (B, H, W, cin, k, fields, st)
    assert lib.eqa_steer_lift_fwd(None, pw, py, pp, *args) == -1
    assert lib.eqa_steer_lift_fwd(px, None, py, pp, *args) == -1
    assert lib.eqa_steer_lift_fwd(px, pw, None, pp, *args) == -1
    assert lib.eqa_steer_lift_fwd(px, pw, py, pp, -1, H, W, cin, k, fields, st) == -1
    assert lib.eqa_steer_lift_fwd(px, pw, py + 4, pp, *args) == -3
    assert lib.eqa_steer_lift_fwd(px, pw, py, pp, 0, H, W, cin, k, fields, st) == 0
    assert lib.eqa_steer_lift_wgrad(None, py, ps, pd, *args) == -1
    assert lib.eqa_steer_lift_wgrad(px, None, ps, pd, *args) == -1
    assert lib.eqa_steer_lift_wgrad(px, py, None, pd, *args) == -1
    assert lib.eqa_steer_lift_wgrad(px, py, ps, None, *args) == -1
    assert lib.eqa_steer_lift_wgrad(px, py, ps, pd, -1, H, W, cin, k, fields, st) == -1
    assert lib.eqa_steer_lift_wgrad(px, py + 4, ps, pd, *args) == -3
    assert lib.eqa_steer_lift_wgrad(px, py, ps, pd, 0, H, W, cin, k, fields, st) == 0
    torch.cuda.synchronize()
    for t in (x, wpk, y, part, ws, dbank):
        assert (t == 5.0).all()                                                          # nothing ran
    good = ops.pack_steer_lift_weights(torch.randn(36, cin, k, k, device=dev))
    with pytest.raises(RuntimeError):
        ops.steer_lift(x.cpu(), good.cpu(), k, fields)
    with pytest.raises(RuntimeError):
        ops.steer_lift(x.contiguous(), good, k, fields)                                  # NCHW with three channels
    with pytest.raises(RuntimeError):
        ops.steer_lift_wgrad(x.contiguous(), y[:B * 49 * 36].view(B, 7, 7, 36).permute(0, 3, 1, 2), k)
    with pytest.raises(_lib.EqaLibraryError):
        ops.steer_lift(x[:, :, :6].contiguous(memory_format=torch.channels_last), good, k, fields)                                     # a map smaller than the filter
    x1 = torch.randn(2, 1, 9, 11, device=dev)                                            # contiguous NCHW, one channel: the same memory
    bank1 = torch.randn(18, 1, 5, 5, device=dev)
    y1, _ = ops.steer_lift(x1, ops.pack_steer_lift_weights(bank1), 5, 2)
    y1_cl, _ = ops.steer_lift(x1.contiguous(memory_format=torch.channels_last), ops.pack_steer_lift_weights(bank1), 5, 2)
    assert torch.equal(y1, y1_cl)
    assert torch.equal(ops.steer_lift_wgrad(x1, y1, 5), ops.steer_lift_wgrad(x1.contiguous(memory_format=torch.channels_last), y1, 5))
