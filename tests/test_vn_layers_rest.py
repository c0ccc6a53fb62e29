"""CPU: VNLinear, VNBilinear, VNSoftplus, VNLeakyReLU and VNStdFeature (the plain route) against vectors the reference itself produced
(tests/golden/vn_layers_rest.pt, written by tests/golden/make_golden_vn_layers_rest.py from the unmodified reference file).

fp64 against the stored fp64 outputs to 1e-12 of the largest value; fp32 at most 4 x as far from the stored fp64 output as the
reference's own stored fp32 output is, that figure pooled over the cases.  Errors are the largest absolute difference over
max(1, largest absolute fp64 value) of the tensor (tests/vn_act_cases.py).
"""
import pytest
import torch

import vn_act_cases as vc

FACTOR = vc.FACTOR
make, rel_error = vc.fixture_module, vc.rel_error


@pytest.fixture(scope="module")
def cases(golden):
    payload = golden("vn_layers_rest.pt")
    assert payload["provenance"] == "reference"
    return payload["cases"]


def layers():
    from equiadapt_amd.pointcloud.canonicalization_networks import vector_neuron_layers

    return vector_neuron_layers


def as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


NAMES = ["linear_4d", "linear_5d", "linear_3d", "leakyrelu_4d", "leakyrelu_shared_5d", "leakyrelu_shared_3d", "softplus_4d",
         "softplus_shared_5d", "bilinear_3d"] + [f"stdfeature_dim{d}_{f}" for d in (3, 4, 5) for f in ("free", "frame")] + ["stdfeature_dim4_train"]


def test_fixture_holds_the_cases(cases):
    assert sorted(cases) == sorted(NAMES)
    assert all(c["inputs"][0].shape[0] in (2, 4) for c in cases.values())


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_matches_the_reference(cases, name):
    case = cases[name]
    mod = getattr(layers(), case["cls"])(*case["args"], **case["kwargs"])
    own = mod.state_dict()
    assert list(own) == list(case["state"])
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in case["state"].items()}
    mod.load_state_dict(case["state"], strict=True)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "bilinear_3d"])      # VNBilinear casts its labels to fp32, as the reference does
def test_fp64_plain_route_reproduces_the_reference(cases, name):
    case = cases[name]
    mod = make(case, torch.float64)
    with torch.no_grad():
        out = mod(*[t.double() for t in case["inputs"]])
    for o, r in zip(as_tuple(out), as_tuple(case["out64"])):
        assert o.dtype == torch.float64 and o.shape == r.shape
        assert float((o - r).abs().max()) <= 1e-12 * float(r.abs().max())
    if hasattr(mod, "last_route"):
        assert mod.last_route.startswith("plain:")


def test_fp32_plain_route_within_four_times_the_reference_fp32_error(cases):
    pooled = vc.fixture_yardstick(cases)
    print(f"reference fp32 error pooled over {len(cases)} cases {pooled:.3e}; budget {FACTOR * pooled:.3e}")
    for name in NAMES:
        case = cases[name]
        with torch.no_grad():
            out = make(case)(*case["inputs"])
        assert all(o.dtype == torch.float32 for o in as_tuple(out))
        err = rel_error(out, case["out64"])
        print(f"{name}: reference fp32 {rel_error(case['out'], case['out64']):.3e}  plain route {err:.3e}")
        assert err <= FACTOR * pooled, name


def test_stdfeature_train_mode_updates_the_running_statistics(cases):
    """A running statistic may be 4 x as far from its fp64 value as the reference's own fp32 one is, or as the pooled output figure
    where that is larger (the reference's fp32 statistic can land on the rounded fp64 value by chance)."""
    case = cases["stdfeature_dim4_train"]
    pooled = vc.fixture_yardstick(cases)
    mod = make(case)
    assert mod.training
    with torch.no_grad():
        out = mod(*case["inputs"])
    assert rel_error(out, case["out64"]) <= FACTOR * pooled
    after = mod.state_dict()
    assert list(after) == list(case["state_after"])
    for k, ref in case["state_after64"].items():
        yard = float((case["state_after"][k].double() - ref).abs().max() / ref.abs().max())
        assert float((after[k].double() - ref).abs().max() / ref.abs().max()) <= FACTOR * max(yard, pooled), k
        assert not torch.equal(after[k], case["state"][k]), k
    for k, v in case["state_after"].items():
        if "num_batches_tracked" in k:
            assert int(after[k]) == int(v) == 1

    mod64 = make(case, torch.float64)
    with torch.no_grad():
        out64 = mod64(case["inputs"][0].double())
    assert rel_error(out64, case["out64"]) <= 1e-12
    for k, ref in case["state_after64"].items():
        assert float((mod64.state_dict()[k] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k


def test_bilinear_raises_on_a_4d_input_like_the_reference():
    mod = layers().VNBilinear(6, 4, 7)
    with pytest.raises(RuntimeError):
        mod(torch.randn(2, 6, 3, 9), torch.randn(2, 1, 4))
    assert mod(torch.randn(2, 6, 3), torch.randn(2, 1, 4)).shape == (2, 7, 3)


def random_orthogonal(seed, proper=False):
    q, r = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)))
    q = q * torch.sign(torch.diagonal(r))
    if proper and torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rotate(x, q):
    return torch.einsum("ij,bcj...->bci...", q, x)


@pytest.mark.parametrize("shape", [(2, 5, 3), (2, 5, 3, 9), (2, 5, 3, 9, 4)])
def test_linear_and_activations_commute_with_orthogonal_maps(shape):
    vnl = layers()
    q = random_orthogonal(7)
    torch.manual_seed(21)
    x = torch.randn(*shape, dtype=torch.float64)
    mods = [vnl.VNLinear(5, 7), vnl.VNLeakyReLU(5), vnl.VNLeakyReLU(5, True, 0.0), vnl.VNSoftplus(5), vnl.VNSoftplus(5, True, 0.1)]
    for qq in (q, random_orthogonal(8), -random_orthogonal(9, proper=True)):      # the last one is improper
        for mod in mods:
            mod = mod.double()
            with torch.no_grad():
                a, b = mod(rotate(x, qq)), rotate(mod(x), qq)
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), type(mod).__name__


@pytest.mark.parametrize("dim,shape", [(3, (4, 8, 3)), (4, (2, 8, 3, 9)), (5, (2, 8, 3, 5, 3))])
def test_stdfeature_with_a_normalised_frame_is_rotation_invariant(dim, shape):
    torch.manual_seed(31 + dim)
    mod = layers().VNStdFeature(8, dim=dim, normalize_frame=True).double().eval()
    x = torch.randn(*shape, dtype=torch.float64)
    q = random_orthogonal(11 + dim, proper=True)
    assert float(torch.det(q)) > 0
    with torch.no_grad():
        (a, za), (b, zb) = mod(rotate(x, q)), mod(x)
    assert a.shape == shape[:2] + (3,) + shape[3:]
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_the_five_names_resolve_from_the_package():
    import equiadapt_amd as ea
    from equiadapt_amd.pointcloud import canonicalization_networks as cn

    for name in ("VNLinear", "VNBilinear", "VNSoftplus", "VNLeakyReLU", "VNStdFeature"):
        assert getattr(ea, name) is getattr(cn, name) is getattr(layers(), name)
        assert name in ea.__all__
    net = ea.VNStdFeature(64, dim=4, normalize_frame=True)
    net.load_state_dict({k: v.clone() for k, v in layers().VNStdFeature(64, dim=4, normalize_frame=True).state_dict().items()}, strict=True)


def test_routes_on_the_cpu_and_the_nbody_classes_are_untouched(monkeypatch):
    from equiadapt_amd.nbody.canonicalization_networks import custom_group_equivariant_layers as nb

    vnl = layers()
    assert nb.VNLeakyReLU is not vnl.VNLeakyReLU and nb.VNSoftplus is not vnl.VNSoftplus
    mod = vnl.VNLeakyReLU(5)
    assert mod.last_route is None
    mod(torch.randn(2, 5, 3, 4))
    assert mod.last_route == "plain: not on the device"
    monkeypatch.setenv("EQA_VN_ACT_KERNEL", "0")
    mod(torch.randn(2, 5, 3, 4))
    assert mod.last_route == "plain: EQA_VN_ACT_KERNEL=0"
