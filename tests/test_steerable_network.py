"""CPU, fp64, plain torch ops: the construction of ESCNNSteerableNetwork (contract, quarter-turn equivariance, centre tap,
FourierELU, dense bank).  This path is the reference the HIP activation kernel is held to in tests/test_gpu_fourier_act.py."""
import math

import pytest
import torch

import equiadapt_amd as ea
from equiadapt_amd.images.canonicalization_networks import steerable_networks as sn

# (in_shape, fields, kernel size, layers): odd size with two hidden layers; even size with the default kernel size
CONFIGS = [((3, 33, 33), 4, 7, 2), ((1, 32, 32), 4, 9, 1)]


def _net(in_shape, fields, k, layers, seed=0):
    torch.manual_seed(seed)
    return ea.ESCNNSteerableNetwork(in_shape, fields, k, "rotation", layers).double()


def _turn(v: torch.Tensor, q: int) -> torch.Tensor:
    """Rows (Re, Im) of v times i^q: the vectors turned by q * 90 degrees (exact: a swap and a sign)."""
    for _ in range(q % 4):
        v = torch.stack([-v[..., 1], v[..., 0]], dim=-1)
    return v


def test_contract_shape_attribute_and_exports():
    net = _net((3, 33, 33), 4, 7, 2)
    assert net.group_type == "rotation"
    out = net(torch.randn(2, 3, 33, 33, dtype=torch.float64))
    assert out.shape == (2, 2, 2) and out.dtype == torch.float64 and torch.isfinite(out).all()
    assert ea.escnn_networks.ESCNNSteerableNetwork is ea.ESCNNSteerableNetwork
    assert "ESCNNSteerableNetwork" in ea.__all__
    # the reference's defaults: kernel_size = 9, one layer
    dflt = ea.ESCNNSteerableNetwork((1, 32, 32), 2)
    assert dflt.kernel_size == 9 and dflt.num_layers == 1 and dflt(torch.randn(1, 1, 32, 32)).shape == (1, 2, 2)


def test_roto_reflection_asserts_with_the_reference_message():
    with pytest.raises(AssertionError, match="group_type must be rotation for now."):
        ea.ESCNNSteerableNetwork((3, 33, 33), 4, 7, "roto-reflection", 1)


def test_state_dict_round_trip_keeps_names_and_output():
    a, b = _net((3, 33, 33), 4, 7, 2, seed=0), _net((3, 33, 33), 4, 7, 2, seed=1)
    sd = a.state_dict()
    assert list(sd) == list(b.state_dict())
    assert list(sd) == [
        "block.0.weights", "block.0.basis", "block.1.weight", "block.1.bias", "block.1.running_mean", "block.1.running_var",
        "block.1.num_batches_tracked", "block.3.weights", "block.3.basis", "block.4.weight", "block.4.bias", "block.4.running_mean",
        "block.4.running_var", "block.4.num_batches_tracked", "block.6.weights", "block.6.basis"]
    assert [n for n, _ in a.named_parameters()] == ["block.0.weights", "block.1.weight", "block.1.bias", "block.3.weights",
                                                     "block.4.weight", "block.4.bias", "block.6.weights"]
    b.load_state_dict(sd)
    x = torch.randn(2, 3, 33, 33, dtype=torch.float64)
    a.eval(), b.eval()
    assert torch.equal(a(x), b(x))


def test_e2cnn_checkpoint_raises_and_says_why():
    net = _net((3, 33, 33), 4, 7, 1)
    bad = {k: v.clone() for k, v in net.state_dict().items()}
    bad["block.0.weights"] = torch.zeros(24)                    # e2cnn: one flat coefficient vector per R2Conv
    with pytest.raises(RuntimeError, match="different function class"):
        net.load_state_dict(bad, strict=False)
    bad = {k: v.clone() for k, v in net.state_dict().items()}
    bad["block.0.basisexpansion.block_expansion_('irrep_0', 'irrep_1').sampled_basis"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="e2cnn"):
        net.load_state_dict(bad, strict=False)


@pytest.mark.parametrize("in_shape,fields,k,layers", CONFIGS)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_quarter_turn_equivariance(in_shape, fields, k, layers, mode):
    """Both rows of net(rot90(x, q)) are the rows of net(x) turned by q * 90 degrees, to 1e-9 of |v|: a property of the
    construction (square grid, rings that depend on r only, zero centre tap).  Measured: 2e-15 .. 5e-15.  In training mode the
    batch statistics are sums over all pixels, which a quarter turn only permutes."""
    net = _net(in_shape, fields, k, layers)
    if mode == "eval":                                          # running statistics that are not the initial 0 / 1
        net.train()
        with torch.no_grad():
            net(torch.randn(2, *in_shape, dtype=torch.float64))
    getattr(net, mode)()
    x = torch.randn(2, *in_shape, dtype=torch.float64)
    with torch.no_grad():
        v = net(x)
        for q in (1, 2, 3):
            vq = net(torch.rot90(x, q, (-2, -1)))
            err = (vq - _turn(v, q)).norm(dim=-1).max() / v.norm(dim=-1).max()
            print(f"{in_shape} k={k} {mode} q={q}: rel err {float(err):.2e}")
            assert float(err) <= 1e-9


@pytest.mark.parametrize("k", [5, 7, 9, 4])
def test_centre_tap_is_zero_for_every_harmonic_but_zero(k):
    basis = sn.SteerableConv(1, "fourier", 1, "fourier", k).double().basis      # (17, J, k, k, 2)
    assert basis.shape == (17, k // 2 + 1, k, k, 2) and basis.dtype == torch.float64
    assert torch.equal(basis, sn.steerable_basis(k))                             # built in fp64, cast: .double() is not an up-cast
    if k % 2:
        c = k // 2
        centre = basis[:, :, c, c, :]
        assert torch.equal(centre[:8], torch.zeros_like(centre[:8])) and torch.equal(centre[9:], torch.zeros_like(centre[9:]))
        assert float(centre[8, 0, 0]) == 1.0 and float(centre[8, 1, 0]) > 0.2    # d = 0 keeps it: ring 1 spills ~0.25 onto r = 0
    for d in range(-8, 9):                                                        # ring j carries |d| <= 2j only
        for j in range(k // 2 + 1):
            if abs(d) > 2 * j:
                assert not basis[d + 8, j].any()


def _field_rotation(t: float) -> torch.Tensor:
    """(9, 9): c_m -> e^{imt} c_m on (a_0, Re c_1, Im c_1, ...)."""
    R = torch.zeros(9, 9, dtype=torch.float64)
    R[0, 0] = 1.0
    for m in range(1, 5):
        c, s = math.cos(m * t), math.sin(m * t)
        R[2 * m - 1, 2 * m - 1], R[2 * m - 1, 2 * m], R[2 * m, 2 * m - 1], R[2 * m, 2 * m] = c, -s, s, c
    return R


def test_fourier_elu_projection_rotation_and_scalar_case():
    A = sn.sampling_matrix()
    assert (A.t() @ A / 16 - torch.eye(9, dtype=torch.float64)).abs().max() <= 1e-14          # A^+ A = I
    act = sn.FourierELU(3).double()
    assert torch.equal(act.A, A)
    torch.manual_seed(0)
    x = 3.0 * torch.randn(2, 27, 5, 4, dtype=torch.float64)
    R = _field_rotation(2.0 * math.pi / 16)

    def rot(t):
        return torch.einsum("ij,bcjhw->bcihw", R, t.unflatten(1, (3, 9))).flatten(1, 2)

    err = (act(rot(x)) - rot(act(x))).abs().max()
    assert float(err) <= 1e-12, float(err)
    # ... and not with a rotation off the 16-point grid (the projection drops what ELU puts above frequency 4)
    R = _field_rotation(0.1)
    assert float((act(rot(x)) - rot(act(x))).abs().max()) > 1e-4
    # a field that has a_0 only: plain ELU on a_0, nothing else appears
    x0 = torch.zeros(2, 27, 5, 4, dtype=torch.float64)
    x0[:, 0::9] = 3.0 * torch.randn(2, 3, 5, 4, dtype=torch.float64)
    y0 = act(x0)
    assert (y0[:, 0::9] - torch.nn.functional.elu(x0[:, 0::9])).abs().max() <= 1e-14
    mask = torch.ones(27, dtype=torch.bool)
    mask[0::9] = False
    assert y0[:, mask].abs().max() <= 1e-14


def test_dense_bank_equals_the_complex_form():
    torch.manual_seed(0)
    conv = sn.SteerableConv(3, "fourier", 2, "fourier", 5).double()
    with torch.no_grad():
        conv.weights.normal_()                                   # every slot, the ones the initialisation leaves at zero included
    x = torch.randn(2, 27, 11, 9, dtype=torch.float64)
    with torch.no_grad():
        dense, cplx = conv(x), conv.complex_forward(x)
    assert dense.shape == (2, 18, 7, 5)
    assert float((dense - cplx).abs().max()) <= 1e-12 * float(dense.abs().max())
    for kinds in (("scalar", "fourier"), ("fourier", "vector"), ("scalar", "vector")):
        conv = sn.SteerableConv(2, kinds[0], 2, kinds[1], 5).double()
        x = torch.randn(1, 2 * conv.in_dim, 8, 8, dtype=torch.float64)
        with torch.no_grad():
            assert float((conv(x) - conv.complex_forward(x)).abs().max()) <= 1e-12 * float(conv(x).abs().max())


def test_initialisation_keeps_the_variance_over_the_fan_in():
    """Unit-variance independent input components -> unit-variance output components, per frequency (SteerableConv docstring).
    16 -> 16 fields, k = 7: 16 * 36 * 36 * 2 samples per component; the estimate's own spread is a few per cent."""
    torch.manual_seed(0)
    conv = sn.SteerableConv(16, "fourier", 16, "fourier", 7).double()
    with torch.no_grad():
        y = conv(torch.randn(2, 144, 42, 42, dtype=torch.float64))
    var = y.unflatten(1, (16, 9)).var(dim=(0, 1, 3, 4))
    assert (var > 0.7).all() and (var < 1.4).all(), var


def test_field_norm_statistics_and_eval_fold():
    torch.manual_seed(0)
    norm = sn.FieldNorm(3).double()
    x = 2.0 * torch.randn(4, 27, 6, 5, dtype=torch.float64) + 0.5
    y = norm(x).unflatten(1, (3, 9))
    assert y[:, :, 0].mean(dim=(0, 2, 3)).abs().max() <= 1e-12                                # frequency 0: batch norm
    assert (y[:, :, 0].var(dim=(0, 2, 3), unbiased=False) - 1.0).abs().max() <= 1e-4
    ms = (y[:, :, 1:] ** 2).unflatten(2, (4, 2)).mean(dim=(0, 3, 4, 5))                       # E[(Re^2 + Im^2) / 2] = 1
    assert (ms - 1.0).abs().max() <= 1e-4
    assert float(norm.num_batches_tracked) == 1 and (norm.running_mean - 0.05).abs().max() < 0.05   # momentum 0.1
    norm.eval()
    scale, shift = norm.folded()
    idx = [0, 1, 1, 2, 2, 3, 3, 4, 4]
    want = x.unflatten(1, (3, 9)) * scale[:, idx][None, :, :, None, None]
    want[:, :, 0] += shift[None, :, None, None]
    assert (norm(x) - want.flatten(1, 2)).abs().max() <= 1e-12
