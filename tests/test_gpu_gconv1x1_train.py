"""eqa_gconv1x1_wgrad (csrc/gconv1x1.hip: filter and bias gradient of the 1 x 1 group convolution) against an fp64 contraction on the
device, and GConv1x1Function against fp64 autograd through F.conv2d."""
import pytest
import torch

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3      # EQA_ERR_UNSUPPORTED (include/eqa_hip.h)
INVALID = -1          # EQA_ERR_INVALID_ARG
U = 2.0 ** -24

# pixel counts off the 16-row stage pair (one row, one short of four stages, ten pairs and a part, 257 splits of one tile) x channel
# pairs with 4-, 8- and 16-byte operand loads (32: one float per lane, 64: two, 96: one again with three tiles, 128: four), Cin != Cout
# both ways; the widest pair (sixteen 128 x 128 tiles) at P = 63
KERNEL_CASES = [(P, ci, co) for P in (1, 63, 162, 4097) for ci, co in ((32, 32), (64, 32), (32, 96), (128, 128))] + [(63, 512, 512)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _operands(dev, P, Cin, Cout, integers=False):
    g = torch.Generator(device=dev).manual_seed(1000 * Cin + Cout + P)
    if integers:
        return (torch.randint(-3, 4, (P, Cin), device=dev, generator=g).float(),
                torch.randint(-3, 4, (P, Cout), device=dev, generator=g).float())
    return torch.randn(P, Cin, device=dev, generator=g), torch.randn(P, Cout, device=dev, generator=g)


def _fp64(x, dz):
    """(dW (Cout, Cin), its magnitude sum, dbias, its magnitude sum) in fp64."""
    xd, zd = x.double(), dz.double()
    return zd.t() @ xd, zd.abs().t() @ xd.abs(), zd.sum(0), zd.abs().sum(0)


@pytest.mark.parametrize("P,Cin,Cout", KERNEL_CASES)
def test_wgrad_stays_inside_the_summation_bound(dev, P, Cin, Cout):
    """Every dW[c][o] within (P + 6) 2^-24 sum_p |x||dz| of the fp64 contraction of the same fp32 operands, every dbias[o] within
    (P + 6) 2^-24 sum_p |dz|: the bound of a P-term sum in any order."""
    from equiadapt_amd import ops

    assert ops.gconv1x1_wgrad_supported(P, Cin, Cout)
    x, dz = _operands(dev, P, Cin, Cout)
    dW, db = ops.gconv1x1_wgrad(x, dz)
    assert dW.shape == (Cout, Cin, 1, 1) and db.shape == (Cout,) and dW.dtype == db.dtype == torch.float32
    want, mag, wantb, magb = _fp64(x, dz)
    err, errb = (dW.view(Cout, Cin).double() - want).abs(), (db.double() - wantb).abs()
    bound, boundb = (P + 6) * U * mag, (P + 6) * U * magb
    print(f"gconv1x1_wgrad P={P} {Cin}->{Cout}: largest error / bound: dW {(err / bound).max().item():.4f}, dbias {(errb / boundb).max().item():.4f}")
    assert bool((err <= bound).all()) and bool((errb <= boundb).all())


@pytest.mark.parametrize("P,Cin,Cout", KERNEL_CASES)
def test_wgrad_is_exact_on_small_integers(dev, P, Cin, Cout):
    """Operands from {-3 .. 3}: every product and partial sum is an integer below 2^24 (4097 x 9), so the result equals the fp64 one
    whatever the order -- a dropped or doubled pixel row shows here."""
    from equiadapt_amd import ops

    x, dz = _operands(dev, P, Cin, Cout, integers=True)
    dW, db = ops.gconv1x1_wgrad(x, dz)
    want, _, wantb, _ = _fp64(x, dz)
    assert torch.equal(dW.view(Cout, Cin).double(), want) and torch.equal(db.double(), wantb)


@pytest.mark.parametrize("P,Cin,Cout", [(1, 32, 32), (63, 64, 32), (162, 32, 96), (4097, 128, 128)])
def test_rows_past_the_pixel_count_are_never_read(dev, P, Cin, Cout):
    """On the first P rows of buffers whose other rows hold 1e30: the same bits as on buffers of P rows."""
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    x, dz = _operands(dev, P, Cin, Cout)
    want_W, want_b = ops.gconv1x1_wgrad(x, dz)
    big_x = torch.cat([x, torch.full((70, Cin), 1e30, device=dev)])
    big_z = torch.cat([dz, torch.full((70, Cout), 1e30, device=dev)])
    dW, db = torch.empty(Cout, Cin, device=dev), torch.empty(Cout, device=dev)
    work = torch.empty(lib.eqa_gconv1x1_wgrad_workspace_bytes(P, Cin, Cout) // 4, device=dev)
    st = lib.eqa_gconv1x1_wgrad(big_x.data_ptr(), big_z.data_ptr(), dW.data_ptr(), db.data_ptr(), work.data_ptr(), P, Cin, Cout, None)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(dW, want_W.view(Cout, Cin)) and torch.equal(db, want_b)


@pytest.mark.parametrize("P,Cin,Cout", [(162, 64, 32), (4097, 128, 128), (63, 512, 512)])
def test_two_launches_give_the_same_bits(dev, P, Cin, Cout):
    from equiadapt_amd import ops

    x, dz = _operands(dev, P, Cin, Cout)
    a, b = ops.gconv1x1_wgrad(x, dz), ops.gconv1x1_wgrad(x, dz)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_map_and_matrix_give_the_same_bits(dev):
    from equiadapt_amd import ops

    x, dz = _operands(dev, 162, 64, 96)
    xm, zm = x.view(2, 9, 9, 64).permute(0, 3, 1, 2), dz.view(2, 9, 9, 96).permute(0, 3, 1, 2)
    a, b = ops.gconv1x1_wgrad(x, dz), ops.gconv1x1_wgrad(xm, zm)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError):
        ops.gconv1x1_wgrad(xm.contiguous(), zm)                             # not channels-last


def test_query_and_launch_agree(dev):
    """Channel counts off the multiples of 32 or above 512, and a map past the 32-bit buffer range: the query says no, the workspace
    query says 0 and the entry point, given no memory at all, answers EQA_ERR_UNSUPPORTED before it looks at a pointer.  P = 0:
    zeros, no workspace.  NULL or aliased pointers: EQA_ERR_INVALID_ARG; a pointer off 16 bytes: EQA_ERR_UNSUPPORTED."""
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    refused = [(100, 48, 64), (100, 64, 544), (2 ** 21, 64, 512), (2 ** 21, 512, 64), (100, 16, 32), (100, 32, 0)]
    for P, ci, co in refused:
        assert not ops.gconv1x1_wgrad_supported(P, ci, co), (P, ci, co)
        assert ops.gconv1x1_wgrad_supported(P, ci, co) == ops.gconv1x1_supported(P, ci, co)
        assert lib.eqa_gconv1x1_wgrad_workspace_bytes(P, ci, co) == 0
    for P, ci, co in refused[:4]:
        assert lib.eqa_gconv1x1_wgrad(None, None, None, None, None, P, ci, co, None) == UNSUPPORTED
    assert ops.gconv1x1_wgrad_supported(2 ** 21 - 1, 64, 512) and ops.gconv1x1_wgrad_supported(0, 32, 32) and ops.gconv1x1_wgrad_supported(7, 512, 512)
    with pytest.raises(_lib.EqaLibraryError):
        ops.gconv1x1_wgrad(torch.zeros(10, 48, device=dev), torch.zeros(10, 64, device=dev))

    dW, db = ops.gconv1x1_wgrad(torch.empty(0, 64, device=dev), torch.empty(0, 32, device=dev))
    assert dW.shape == (32, 64, 1, 1) and not bool(dW.any()) and not bool(db.any())

    x, dz = _operands(dev, 20, 32, 32)
    out = torch.empty(32 * 32 + 32 + 8, device=dev)
    work = torch.empty(lib.eqa_gconv1x1_wgrad_workspace_bytes(20, 32, 32) // 4, device=dev)
    pw, pb = out.data_ptr(), out.data_ptr() + 32 * 32 * 4
    assert lib.eqa_gconv1x1_wgrad(x.data_ptr(), dz.data_ptr(), pw, pb, work.data_ptr(), 20, 32, 32, None) == 0
    assert lib.eqa_gconv1x1_wgrad(None, dz.data_ptr(), pw, pb, work.data_ptr(), 20, 32, 32, None) == INVALID
    assert lib.eqa_gconv1x1_wgrad(x.data_ptr(), dz.data_ptr(), pw, pb, None, 20, 32, 32, None) == INVALID
    assert lib.eqa_gconv1x1_wgrad(x.data_ptr(), dz.data_ptr(), x.data_ptr(), pb, work.data_ptr(), 20, 32, 32, None) == INVALID
    assert lib.eqa_gconv1x1_wgrad(x.data_ptr(), dz.data_ptr(), pw, pb + 4, work.data_ptr(), 20, 32, 32, None) == UNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.parametrize("Cin,Cout", [(64, 32), (128, 128)])
def test_function_against_fp64_autograd(dev, Cin, Cout):
    """GConv1x1Function(x, bank, bias, res) at P = 162 against fp64 autograd through F.conv2d(x, bank) + bias + res: the output and
    dx, dbank, dbias inside the dot-product bounds (Cin + 6 terms for the output, Cout + 6 for dx, P + 6 for dbank and dbias),
    dres bit-equal to the incoming gradient."""
    import torch.nn.functional as F

    from equiadapt_amd.images.canonicalization_networks.wrn_networks import GConv1x1Function

    g = torch.Generator(device=dev).manual_seed(Cin + Cout)
    nhwc = torch.channels_last
    P = 162
    x = torch.randn(2, Cin, 9, 9, device=dev, generator=g).contiguous(memory_format=nhwc).requires_grad_()
    res = torch.randn(2, Cout, 9, 9, device=dev, generator=g).contiguous(memory_format=nhwc).requires_grad_()
    bank = (torch.randn(Cout, Cin, 1, 1, device=dev, generator=g) / Cin ** 0.5).requires_grad_()
    bias = torch.randn(Cout, device=dev, generator=g).requires_grad_()
    dy = torch.randn(2, Cout, 9, 9, device=dev, generator=g).contiguous(memory_format=nhwc)

    y = GConv1x1Function.apply(x, bank, bias, res)
    assert y.shape == dy.shape and y.is_contiguous(memory_format=nhwc)
    y.backward(dy)
    x64, r64, w64, b64 = (t.detach().double().requires_grad_() for t in (x, res, bank, bias))
    y64 = F.conv2d(x64, w64) + b64[None, :, None, None] + r64
    y64.backward(dy.double())

    def rows(t):
        return t.detach().double().permute(0, 2, 3, 1).reshape(P, -1)

    xa, wa, da = rows(x).abs(), w64.detach().abs().view(Cout, Cin), rows(dy).abs()
    checks = {
        "y": (rows(y), rows(y64), (Cin + 6) * U * (xa @ wa.t() + b64.detach().abs() + rows(res).abs())),
        "dx": (rows(x.grad), rows(x64.grad), (Cout + 6) * U * (da @ wa)),
        "dbank": (bank.grad.double().view(Cout, Cin), w64.grad.view(Cout, Cin), (P + 6) * U * (da.t() @ xa)),
        "dbias": (bias.grad.double(), b64.grad, (P + 6) * U * da.sum(0)),
    }
    for name, (got, want, bound) in checks.items():
        err = (got - want).abs()
        print(f"GConv1x1Function {Cin}->{Cout} {name}: largest error / bound {(err / bound).max().item():.4f}")
        assert bool((err <= bound).all()), name
    assert torch.equal(res.grad, dy)

    # without a residual, and with only the bank asking for a gradient: the same filter gradient once more (x + x is exact)
    g1, gb = bank.grad.clone(), bias.grad.clone()
    GConv1x1Function.apply(x.detach(), bank, bias.detach(), None).backward(dy)
    assert torch.equal(bank.grad, 2 * g1) and torch.equal(bias.grad, gb)
