"""eqa_window_sums_tail: window-sum partials -> (activations, first-maximum index, rotation, reflection) in one launch, one block per
image, against the launches it replaces on the SAME inverse transform: eqa_fft48k5_output_sums (finalize kernel) ->
ops.window_sums_gemv -> ops.group_argmax -> torch.index_select.  Every addition is meant to be made in the order those kernels make it,
so the comparison is torch.equal, not a tolerance.

What can go wrong: the segment walk (border pieces first in fp32, then the fp64 chain) for a piece count that is no multiple of the
eight-piece batches; the window assembly indexing another channel's border rows (the strides differ from the finalize kernel's 32-channel
blocks); the GEMV's partition when its 1024 threads are dealt over (column slot, activation) instead of 256 over columns; E not a multiple
of the four activation groups; an index past E from the padding lanes of the argmax.  OH = OW: 9 (the smallest map a k = 5 tail admits),
44 (one tile), 45 (a one-pixel second tile: `sub` = 2 and ragged pieces), 88 (the headline's 2 x 2)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _inverse(dev, nimg, OH, C, k, want_S):
    """One inverse transform of random spectra up to S (eqa_fft48k5_output_sums) or up to the partials (-> part, pieces, sub)."""
    import ctypes

    from equiadapt_amd import _lib, ops
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    TX = fftconv.tiles(OH + 4)
    M = nimg * TX * TX
    torch.manual_seed(nimg * 1000 + OH * 10 + C + k)
    Mo = fftconv.spectra_buffer(M, 2 * C, dev)
    Mo.copy_(torch.randn(Mo.shape, device=dev))
    bias = torch.randn(C, device=dev)
    T2 = fftconv._workspace(5, nimg, OH, OH, C, dev)
    ws = torch.full((nimg * OH * TX * C * (2 * k - 1),), float("nan"), dtype=torch.float32, device=dev)
    st = ops._stream()
    if want_S:
        S = torch.empty((nimg, C, k, k), dtype=torch.float64, device=dev)
        _lib.check(lib.eqa_fft48k5_output_sums(Mo.data_ptr(), T2.data_ptr(), bias.data_ptr(), 1, S.data_ptr(), ws.data_ptr(), nimg, OH, OH, C, k,
                                               st), "eqa_fft48k5_output_sums")
        return S
    ns = (ctypes.c_int * 2)()
    _lib.check(lib.eqa_fft48k5_output_sums_partials(Mo.data_ptr(), T2.data_ptr(), bias.data_ptr(), 1, ws.data_ptr(), nimg, OH, OH, C, k, ns,
                                                    st), "eqa_fft48k5_output_sums_partials")
    return ws, ns[0], ns[1]


def _tables(E, dev, reflections):
    rot = torch.linspace(0.0, 360.0, E + 1)[:E].to(dev)
    return rot, (torch.arange(E) >= E // 2).float().to(dev) if reflections else None


def _reference(S, Wm, scale, shift, rot, ref):
    from equiadapt_amd import ops

    act = ops.window_sums_gemv(S.flatten(1), Wm, scale, shift)
    gidx = ops.group_argmax(act)
    return act, gidx, torch.index_select(rot, 0, gidx), (torch.index_select(ref, 0, gidx) if ref is not None else None)


def _same(got, want):
    for g, w, name in zip(got, want, ("activations", "index", "rotation", "reflection")):
        assert (g is None) == (w is None), name
        if g is not None:
            assert g.dtype == w.dtype and torch.equal(g, w), name


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("OH", [9, 44, 45, 88])
@pytest.mark.parametrize("nimg", [1, 3])
def test_tail_equals_the_launches_it_replaces(dev, nimg, OH, C, k):
    from equiadapt_amd import ops

    S = _inverse(dev, nimg, OH, C, k, True)
    part, pieces, sub = _inverse(dev, nimg, OH, C, k, False)
    assert pieces % sub == 0 and pieces // sub >= 2 * (k - 1) + 1
    scale, shift = 1.0 / (32 * (OH - k + 1) ** 2), 0.125
    for E in (4, 8, 16):
        assert ops.window_sums_tail_supported(C, k, E)
        Wm = torch.randn(E, C * k * k, dtype=torch.float64, device=dev)
        rot, ref = _tables(E, dev, reflections=E == 16)
        want = _reference(S, Wm, scale, shift, rot, ref)
        got = ops.window_sums_tail(part, nimg, C, k, pieces, sub, Wm, scale, shift, rot, ref)
        _same(got, want)
        assert int(got[1].min()) >= 0 and int(got[1].max()) < E


@pytest.mark.parametrize("k,OH,C", [(5, 88, 256), (3, 45, 32)])
def test_a_tie_returns_the_first_index(dev, k, OH, C):
    from equiadapt_amd import ops

    S = _inverse(dev, 1, OH, C, k, True)
    part, pieces, sub = _inverse(dev, 1, OH, C, k, False)
    E, scale, shift = 8, 1.0 / (32 * (OH - k + 1) ** 2), 0.0
    rot, ref = _tables(E, dev, False)
    Wm = torch.randn(E, C * k * k, dtype=torch.float64, device=dev)
    m = int(ops.group_argmax(ops.window_sums_gemv(S.flatten(1), Wm, scale, shift))[0])
    lo, hi = (m, 7) if m < 7 else (2, 7)
    Wm[lo] = Wm[m]
    Wm[hi] = Wm[m]                                    # equal rows: equal activations, bit for bit, and the largest
    want = _reference(S, Wm, scale, shift, rot, ref)
    got = ops.window_sums_tail(part, 1, C, k, pieces, sub, Wm, scale, shift, rot, ref)
    _same(got, want)
    assert got[0][0, lo].item() == got[0][0, hi].item() == got[0].max().item()
    assert int(got[1][0]) == lo and got[2][0].item() == rot[lo].item()
    Wm[:] = Wm[0]                                     # every activation equal: index 0
    got = ops.window_sums_tail(part, 1, C, k, pieces, sub, Wm, scale, shift, rot, ref)
    _same(got, _reference(S, Wm, scale, shift, rot, ref))
    assert int(got[1][0]) == 0


def test_refusals(dev):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    nimg, C, k, E = 1, 32, 5, 8
    part, pieces, sub = _inverse(dev, nimg, 44, C, k, False)
    Wm = torch.randn(E, C * k * k, dtype=torch.float64, device=dev)
    rot, ref = _tables(E, dev, True)
    act, gidx = torch.empty(nimg, E, device=dev), torch.empty(nimg, dtype=torch.int32, device=dev)
    r1, r2 = torch.empty(nimg, device=dev), torch.empty(nimg, device=dev)
    ptrs = [part.data_ptr(), Wm.data_ptr(), act.data_ptr(), gidx.data_ptr(), rot.data_ptr(), ref.data_ptr(), r1.data_ptr(), r2.data_ptr()]

    def call(p=ptrs, C=C, k=k, pieces=pieces, sub=sub, E=E, B=nimg):
        return lib.eqa_window_sums_tail(*p, B, C, k, pieces, sub, E, 1.0, 0.0, None)

    assert call() == 0
    torch.cuda.synchronize()
    for i in (0, 1, 2, 3, 4, 6):
        assert call(p=ptrs[:i] + [None] + ptrs[i + 1:]) == -1
    assert call(p=ptrs[:7] + [None]) == -1                       # a reflection table without its output
    assert call(p=ptrs[:5] + [None, ptrs[6], None]) == 0         # no reflection table: a rotation group
    torch.cuda.synchronize()
    assert call(E=0) == -1 and call(C=0) == -1 and call(sub=0) == -1 and call(pieces=2 * (k - 1) * sub) == -1 and call(pieces=21, sub=2) == -1
    assert call(B=0) == 0
    assert call(E=17) == -3 and call(k=4, pieces=100) == -3 and call(k=7, pieces=100) == -3 and call(C=512) == -3
    assert not ops.window_sums_tail_supported(512, 5, 8) and ops.window_sums_tail_supported(256, 5, 16) and not ops.window_sums_tail_supported(256, 5, 17)
