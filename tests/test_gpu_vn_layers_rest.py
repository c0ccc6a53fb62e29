"""GPU: the fused route of VNLeakyReLU / VNSoftplus (eqa_vn_act_fwd / _bwd) against the fp64 CPU plain route, and VNStdFeature on the device.

Budget (tests/vn_act_cases.py): the fused route's error may be at most 4 x the error of torch's fp32 CPU plain route against the same
fp64 result, that figure computed here and pooled over the cases; VNStdFeature's fixture cases are held to 4 x the pooled error of
the reference's own stored fp32 outputs.  Every figure is printed before it is asserted (-s shows them).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import vn_act_cases as vc  # noqa: E402

FACTOR = vc.FACTOR
INVALID, UNSUPPORTED = -1, -3      # EQA_ERR_INVALID_ARG, EQA_ERR_UNSUPPORTED (include/eqa_hip.h)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def on_device(t, dev):
    """A copy of t in a device buffer that torch.empty hands out (so that the guard bands of tests/conftest.py surround it)."""
    out = torch.empty(tuple(t.shape), dtype=t.dtype, device=dev)
    out.copy_(t)
    return out


def build_on_device(c, dev):
    mod, x, r = vc.build(c, torch.float32, "cpu")
    return mod.to(dev), on_device(x, dev), on_device(r, dev)


@pytest.fixture(scope="module")
def forward_refs():
    """name -> (fp64 output, fp32 CPU error); and the pooled fp32 figure."""
    refs = {}
    for c in vc.FORWARD_CASES:
        m64, x64, _ = vc.build(c, torch.float64, "cpu")
        m32, x32, _ = vc.build(c, torch.float32, "cpu")
        with torch.no_grad():
            ref = m64(x64)
            refs[c["name"]] = (ref, vc.rel_error(m32(x32), ref))
    pooled = max(e for _, e in refs.values())
    print(f"forward: fp32 CPU error pooled over {len(refs)} cases {pooled:.3e}; budget {FACTOR * pooled:.3e}")
    return refs, pooled


@pytest.fixture(scope="module")
def backward_refs():
    """name -> (loss weights in fp64, fp64 (gx, gW), fp32 CPU errors, dropped share); and the pooled fp32 figure."""
    refs = {}
    for c in vc.BACKWARD_CASES:
        m64, x64, r64 = vc.build(c, torch.float64, "cpu")
        m32, x32, _ = vc.build(c, torch.float32, "cpu")
        keep = torch.ones_like(r64[:, :, :1]) if c["softplus"] else vc.kink_free(c)
        w64 = r64 * keep
        g64 = vc.gradients(m64, x64, w64)
        g32 = vc.gradients(m32, x32, w64.float())
        refs[c["name"]] = (w64, g64, tuple(vc.rel_error(a, b) for a, b in zip(g32, g64)), 1.0 - float(keep.mean()))
    pooled = max(max(e) for _, _, e, _ in refs.values())
    print(f"backward: fp32 CPU error pooled over {len(refs)} cases {pooled:.3e}; budget {FACTOR * pooled:.3e}")
    return refs, pooled


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", vc.FORWARD_CASES, ids=[c["name"] for c in vc.FORWARD_CASES])
def test_fused_forward_within_four_times_the_fp32_cpu_error(c, forward_refs, dev):
    refs, pooled = forward_refs
    ref, e32 = refs[c["name"]]
    mod, x, _ = build_on_device(c, dev)
    with torch.no_grad():
        y = mod(x)
    assert mod.last_route == "fused", mod.last_route
    assert y.shape == ref.shape and y.dtype == torch.float32
    err = vc.rel_error(y, ref)
    print(f"forward {c['name']}: fp32 CPU {e32:.3e}  fused {err:.3e}  ratio to pooled fp32 {err / pooled:.2f}")
    assert err <= FACTOR * pooled


def test_a_non_contiguous_input_is_made_contiguous(forward_refs, dev):
    refs, pooled = forward_refs
    c = next(c for c in vc.FORWARD_CASES if c["C"] == 21 and len(c["shape"]) == 5)
    mod, x, _ = build_on_device(c, dev)
    xt = on_device(x.transpose(3, 4).contiguous(), dev).transpose(3, 4)
    assert not xt.is_contiguous()
    with torch.no_grad():
        y = mod(xt)
    assert mod.last_route == "fused"
    assert vc.rel_error(y, refs[c["name"]][0]) <= FACTOR * pooled


@pytest.mark.parametrize("name", ["leakyrelu_4d", "leakyrelu_shared_5d", "leakyrelu_shared_3d", "softplus_4d", "softplus_shared_5d"])
def test_fixture_activations_on_the_device(golden, name, forward_refs, dev):
    _, pooled = forward_refs
    case = golden("vn_layers_rest.pt")["cases"][name]
    mod = vc.fixture_module(case).to(dev)
    with torch.no_grad():
        y = mod(on_device(case["inputs"][0], dev))
    assert mod.last_route == "fused"
    err = vc.rel_error(y, case["out64"])
    print(f"fixture {name}: reference fp32 {vc.rel_error(case['out'], case['out64']):.3e}  fused {err:.3e}  pooled fp32 CPU {pooled:.3e}")
    assert err <= FACTOR * pooled


# --------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("c", vc.BACKWARD_CASES, ids=[c["name"] for c in vc.BACKWARD_CASES])
def test_fused_gradients_within_four_times_the_fp32_cpu_error(c, backward_refs, dev):
    refs, pooled = backward_refs
    w64, g64, e32, dropped = refs[c["name"]]
    print(f"backward {c['name']}: share of (b, c, p) without loss weight {dropped:.2e}")
    assert dropped <= vc.MAX_DROPPED
    mod, x, _ = build_on_device(c, dev)
    gx, gW = vc.gradients(mod, x, on_device(w64.float(), dev))
    assert mod.last_route == "fused", mod.last_route
    assert gx.shape == g64[0].shape and gW.shape == g64[1].shape
    errs = (vc.rel_error(gx, g64[0]), vc.rel_error(gW, g64[1]))
    print(f"backward {c['name']}: gx fp32 CPU {e32[0]:.3e} fused {errs[0]:.3e}; dL/dWd fp32 CPU {e32[1]:.3e} fused {errs[1]:.3e}; "
          f"ratio to pooled fp32 {max(errs) / pooled:.2f}")
    assert errs[0] <= FACTOR * pooled
    assert errs[1] <= FACTOR * pooled


@pytest.mark.parametrize("c", vc.SOFTPLUS_C1_CASES, ids=[c["name"] for c in vc.SOFTPLUS_C1_CASES])
def test_softplus_gradients_are_finite_where_the_direction_is_parallel(c, dev):
    """C = 1: d = w x is parallel to x at every point; the plain route's gradient through acos (the reference's) is not finite there."""
    mod, x, r = build_on_device(c, dev)
    gx, gW = vc.gradients(mod, x, r)
    assert mod.last_route == "fused"
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gW).all())


def test_two_backward_launches_give_the_same_bits(dev):
    for c in (vc.BACKWARD_CASES[8], vc.BACKWARD_CASES[4], vc.BACKWARD_CASES[13]):       # C = 85 own, C = 21 shared, softplus shared
        mod, x, r = build_on_device(c, dev)
        gx1, gW1 = vc.gradients(mod, x, r)
        gx2, gW2 = vc.gradients(mod, x, r)
        assert mod.last_route == "fused"
        assert torch.equal(gx1, gx2) and torch.equal(gW1, gW2), c["name"]


def test_both_kernels_can_be_captured_into_a_graph(dev):
    """No host synchronisation on the fused route: a captured forward and backward replay to the bits of the eager calls."""
    from equiadapt_amd import ops

    c = vc.BACKWARD_CASES[5]                                             # C = 21, (2, 21, 3, 257)
    mod, x, r = build_on_device(c, dev)
    W = mod.map_to_dir.weight.detach()
    with torch.no_grad():
        y_eager = mod(x)
        gx_eager, gW_eager = ops.vn_act_backward(x, W, r, c["softplus"], c["slope"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y = mod(x)
        gx, gW = ops.vn_act_backward(x, W, r, c["softplus"], c["slope"])
    assert mod.last_route == "fused"
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, y_eager) and torch.equal(gx, gx_eager) and torch.equal(gW, gW_eager)


# ---------------------------------------------------------------------------------------------------------------- routes
def test_routes(monkeypatch, forward_refs, dev):
    from equiadapt_amd import _lib
    from equiadapt_amd.pointcloud.canonicalization_networks import VNLeakyReLU

    _, pooled = forward_refs
    limit = _lib.load().eqa_vn_act_max_channels()
    assert limit >= 85
    wide = vc.case(limit + 1, (2, 65), False, False, 0.2, 130)
    m64, x64, _ = vc.build(wide, torch.float64, "cpu")
    mod, x, _ = build_on_device(wide, dev)
    with torch.no_grad():
        ref, y = m64(x64), mod(x)
    assert mod.last_route.startswith("plain:") and str(limit) in mod.last_route
    assert vc.rel_error(y, ref) <= FACTOR * pooled

    c = vc.FORWARD_CASES[8]
    mod, x, _ = build_on_device(c, dev)
    mod(x)
    assert mod.last_route == "fused"
    mod.double()(x.double())
    assert mod.last_route.startswith("plain:") and "float64" in mod.last_route
    mod.float()
    monkeypatch.setenv("EQA_VN_ACT_KERNEL", "0")
    with torch.no_grad():
        y = mod(x)
    assert mod.last_route == "plain: EQA_VN_ACT_KERNEL=0"
    assert vc.rel_error(y, forward_refs[0][c["name"]][0]) <= FACTOR * pooled
    monkeypatch.delenv("EQA_VN_ACT_KERNEL")
    empty = VNLeakyReLU(5).to(dev)
    assert empty(torch.empty(0, 5, 3, 4, device=dev)).shape == (0, 5, 3, 4)
    assert empty.last_route.startswith("plain:")


def test_argument_errors(dev):
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    limit = lib.eqa_vn_act_max_channels()
    assert lib.eqa_vn_act_bwd_blocks(0) == INVALID and lib.eqa_vn_act_bwd_blocks(-5) == INVALID
    assert lib.eqa_vn_act_bwd_blocks(1) == 1
    assert 0 < lib.eqa_vn_act_bwd_blocks(1 << 40) <= 1024
    C = 5
    x = torch.zeros(2, C, 3, 8, dtype=torch.float32, device=dev)
    W = torch.zeros(C, C, dtype=torch.float32, device=dev)
    y = torch.zeros(2, C, 3, 8, dtype=torch.float32, device=dev)
    part = torch.zeros(lib.eqa_vn_act_bwd_blocks(16), C, C, dtype=torch.float32, device=dev)
    px, pW, py, pp = x.data_ptr(), W.data_ptr(), y.data_ptr(), part.data_ptr()

    def fwd(px=px, pW=pW, py=py, B=2, C=C, P=8, D=C):
        return lib.eqa_vn_act_fwd(px, pW, py, B, C, P, D, 0, 0.2, None)

    def bwd(px=px, pW=pW, pg=py, pgx=py, pp=pp, B=2, C=C, P=8, D=C):
        return lib.eqa_vn_act_bwd(px, pW, pg, pgx, pp, B, C, P, D, 1, 0.0, None)

    for call in (fwd, bwd):
        assert call(px=None) == INVALID and call(pW=None) == INVALID
        assert call(B=0) == INVALID and call(C=0) == INVALID and call(P=0) == INVALID and call(B=-1) == INVALID
        assert call(D=2) == INVALID and call(D=0) == INVALID
        assert call(C=limit + 1, D=limit + 1) == UNSUPPORTED and call(C=limit + 1, D=1) == UNSUPPORTED
    assert fwd(py=None) == INVALID
    assert bwd(pg=None) == INVALID and bwd(pgx=None) == INVALID and bwd(pp=None) == INVALID
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0 and float(part.abs().max()) == 0.0          # nothing was launched

    with pytest.raises(RuntimeError):
        ops.vn_act(torch.zeros(2, C, 3, 8), torch.zeros(C, C), False, 0.2)
    with pytest.raises(RuntimeError):
        ops.vn_act_backward(torch.zeros(2, C, 3, 8), torch.zeros(C, C), torch.zeros(2, C, 3, 8), False, 0.2)
    with pytest.raises(ValueError):
        ops.vn_act(x, torch.zeros(2, C, dtype=torch.float32, device=dev), False, 0.2)
    assert ctypes.sizeof(ctypes.c_longlong) == 8


# ----------------------------------------------------------------------------------------------------------- VNStdFeature
@pytest.mark.parametrize("name", ["stdfeature_dim4_free", "stdfeature_dim4_frame", "stdfeature_dim4_train"])
def test_stdfeature_on_the_device(golden, name, dev):
    cases = golden("vn_layers_rest.pt")["cases"]
    pooled = vc.fixture_yardstick(cases)
    case = cases[name]
    mod = vc.fixture_module(case).to(dev)
    assert mod.training == case["train"]
    with torch.no_grad():
        out = mod(on_device(case["inputs"][0], dev))
    err = vc.rel_error(out, case["out64"])
    print(f"{name}: reference fp32 {vc.rel_error(case['out'], case['out64']):.3e}  device {err:.3e}  pooled {pooled:.3e}")
    assert err <= FACTOR * pooled
    if case["train"]:
        after = mod.state_dict()
        for k, ref in case["state_after64"].items():
            yard = float((case["state_after"][k].double() - ref).abs().max() / ref.abs().max())
            assert float((after[k].double().cpu() - ref).abs().max() / ref.abs().max()) <= FACTOR * max(yard, pooled), k
