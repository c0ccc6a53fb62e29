"""CPU: the fp64 reference of the group action (oracle/action_fp64.py) and the comparison that
tests/test_gpu_action_backward_fp64.py makes with it.

1. Conventions.  The reference is a function of the kernel's arguments (tables, flags, channel maps, crop); run in fp32 on the
   package's own group tables it must reproduce the project's oracle of the group (oracle/image_ops.py), to the oracle's own fp32
   level.  That pins the flags, the sign of the angle, the channel map and the crop.
2. Planted errors.  The measures and budgets of tests/action_backward_cases.py are fed the fp32 CPU chain's result with ONE defect
   of the kind a kernel could have; each must exceed its budget at least ten times.  A check that cannot fail holds nothing.
"""
import math

import pytest
import torch

import action_backward_cases as ac
from equiadapt_amd.images import geometry
from oracle import action_fp64 as ref
from oracle import image_ops as io

FIRST, FOURTH, LAST = ac.CASES[0].name, ac.CASES[3].name, ac.CASES[-1].name


# ---- 1. conventions -------------------------------------------------------------------------------------------------------


def _agrees_with_oracle(got32, oracle, got64):
    """Two fp32 evaluations of one expression: they may differ by what either differs from fp64 (4 x, the order of the
    operations), and by no less than a few ulps of the values."""
    level = max((oracle.double() - got64).abs().max().item(), 4 * torch.finfo(torch.float32).eps * got64.abs().max().item())
    err = (got32.double() - oracle.double()).abs().max().item()
    assert err <= 4 * level, (err, level)
    assert level <= 1e-4 * got64.abs().max().item(), level        # and the oracle itself is an fp32 evaluation of the reference


@pytest.mark.parametrize("N,refl", [(8, False), (4, True)])
def test_reference_reproduces_the_oracle_canonicalization(N, refl):
    C, H, W = 3, 33, 47
    G = 2 * N if refl else N
    torch.manual_seed(N)
    gidx = torch.cat([torch.arange(G), torch.tensor([1, G - 1])]).to(torch.int32)
    x = torch.randn(gidx.shape[0], C, H, W)
    pad = math.ceil(W * 0.5)
    theta, flags = geometry.canonicalize_tables(N, refl, (H + 2 * pad, W + 2 * pad))
    rot = io.group_angles(N)[gidx.long() % N]
    want = io.canonicalize_images(x, rot, (gidx >= N).float() if refl else None, (C, H, W))
    args = (x, gidx, theta, flags, None, pad, (H, W), (pad, pad))
    _agrees_with_oracle(ref.action(*args, dtype=torch.float32).out, want, ref.action(*args, dtype=torch.float64).out)


@pytest.mark.parametrize("N,refl,rep", [(8, False, "scalar"), (8, False, "regular"), (4, True, "scalar"), (4, True, "regular")])
def test_reference_reproduces_the_oracle_inverse_action(N, refl, rep):
    H, W = 40, 56
    G = 2 * N if refl else N
    C = 2 * G if rep == "regular" else 3
    torch.manual_seed(10 + N)
    gidx = torch.cat([torch.arange(G), torch.tensor([1, G - 1])]).to(torch.int32)
    f = torch.randn(gidx.shape[0], C, H, W)
    theta, flags, cmap = geometry.invert_tables(N, refl, (H, W))
    rot = io.group_angles(N)[gidx.long() % N]
    want = io.invert_action(f, rot, (gidx >= N).float() if refl else None, N, G, rep)
    args = (f, gidx, theta, flags, cmap if rep == "regular" else None, 0, (H, W), (0, 0))
    _agrees_with_oracle(ref.action(*args, dtype=torch.float32).out, want, ref.action(*args, dtype=torch.float64).out)


def test_reference_rotation_theta_is_the_tables():
    """The fp64 restatement whose Jacobian turns dL/dtheta into dL/d angle reproduces the fp32 tables the kernels get, and its
    Jacobian is the derivative of those tables (central difference in fp64)."""
    for case in ac.CASES:
        fr, a = ac.frame_hw(case), ac.angles_of(case)
        assert (ref.rotation_theta(a, fr).float() - geometry.rotation_theta(a, fr)).abs().max().item() <= 1e-6
        h = 1e-4
        fd = (ref.rotation_theta(a.double() + h, fr) - ref.rotation_theta(a.double() - h, fr)) / (2 * h)
        jac = ref.rotation_theta_jacobian(a, fr)
        assert (fd - jac).abs().max().item() <= 1e-8 * max(1.0, jac.abs().max().item())


def test_inputs_keep_off_the_kinks():
    """The conditions on the inputs, on the reference alone: even frames, no right angle, at most 3 % of any image's output
    pixels zeroed -- and no kept pixel's sample point within 2**-9 px of a grid line."""
    for case in ac.CASES:
        for rows in ("rotation",) + (("affine",) if case.theta_case else ()):
            share = ac.check_inputs_are_unambiguous(case.name, rows)
            assert 0.0 < share <= ac.MAX_ZEROED
            s = ac.setup(case, rows)
            src, gy, _ = ac.smooth_inputs(case.name, rows)
            res = ref.action(src, s.gidx, s.theta, s.flags, s.chan_map, case.pad, case.out_hw, case.top_left)
            kept = (gy != 0).any(dim=1)
            frac = torch.stack([res.ix - res.ix.floor(), res.iy - res.iy.floor()])
            assert torch.minimum(frac, 1 - frac)[:, kept].min().item() >= ac.KINK_MARGIN


# ---- 2. planted errors ----------------------------------------------------------------------------------------------------


def _chain32(case_name, rows, inputs, **changed):
    """The fp32 CPU chain on a case's inputs with some arguments of the call replaced."""
    c = ac.CASE_BY_NAME[case_name]
    s = ac.setup(c, rows)._replace(**{k: v for k, v in changed.items() if k in ("flags", "chan_map", "theta")})
    src, gy = inputs[0], changed.get("grad_out", inputs[1])
    return ref.action_grads(src, gy, s.gidx, s.theta, s.flags, s.chan_map, c.pad, changed.get("top_left", c.top_left),
                            dtype=torch.float32)


def _angle_error(name, d_theta, jac=None):
    want = ac.angle_gradient(ac.transform_gradient_reference(name, "rotation").f64.d_theta, ac.angle_jacobian(name))
    return ac.measure_per_image(ac.angle_gradient(d_theta, ac.angle_jacobian(name) if jac is None else jac), want)


def _caught(err, quantity):
    assert err >= 10 * ac.budgets()[quantity], (quantity, err, ac.budgets()[quantity])


def test_budgets_are_fp32_rounding_errors():
    """The pooled budgets are fp32 rounding errors times M.  Measured on two hosts (their BLAS evaluate affine_grid differently):
    1.5 - 1.6e-4 for the input gradient's interior (a coordinate error of ~3e-5 px on white noise), 0.8 - 2.1e-5 for the angle and
    2.4 - 2.7e-5 for the theta gradient.  The upper bounds here are ten times those: the budgets come from the chain, this only
    guards against a reference that has quietly become loose -- a kink that is no longer masked costs 2e-3."""
    b = ac.budgets()
    assert b["input:interior"] <= 2e-3 and b["input:borders"] <= 2e-3 and b["input:corners"] <= 2e-3
    assert b["angle"] <= 2e-4 and b["theta"] <= 3e-4 and b["forward"] <= 1e-3
    assert all(v > 0 for v in b.values())
    # and the chain passes its own check, case by case
    for key, v in ac.cpu_chain_errors().items():
        assert v <= b[key[0]] / ac.M_BUDGET


@pytest.mark.parametrize("name", [FIRST, FOURTH, LAST])
def test_planted_rotation_centre_off_by_half_a_pixel(name):
    c = ac.CASE_BY_NAME[name]
    Hp, Wp = ac.frame_hw(c)
    jac = ref.rotation_theta_jacobian(ac.angles_of(c), (Hp, Wp), center=((Wp - 1) / 2.0 + 0.5, (Hp - 1) / 2.0))
    _caught(_angle_error(name, ac.transform_gradient_reference(name, "rotation").f32.d_theta, jac), "angle")


@pytest.mark.parametrize("name", [FIRST, FOURTH])
def test_planted_half_w_and_half_h_exchanged(name):
    """(the last case's frame is square: the exchange is the identity there)"""
    c = ac.CASE_BY_NAME[name]
    Hp, Wp = ac.frame_hw(c)
    assert Hp != Wp and ac.frame_hw(ac.CASE_BY_NAME[LAST])[0] == ac.frame_hw(ac.CASE_BY_NAME[LAST])[1]
    t = ac.transform_gradient_reference(name, "rotation")
    d = t.f32.d_theta.clone()
    d[:, :3] *= (Hp - 1.0) / (Wp - 1.0)
    d[:, 3:] *= (Wp - 1.0) / (Hp - 1.0)
    _caught(ac.measure_theta_gradient(d, t.f64.d_theta), "theta")


@pytest.mark.parametrize("name", [FIRST, FOURTH, LAST])
def test_planted_dropped_tile_in_the_angle_gradient(name):
    src, gy, _ = ac.smooth_inputs(name, "rotation")
    gy = gy.clone()
    gy[:, :, 32:64, 32:64] = 0.0                      # tile (1, 1) of every image contributes nothing
    _caught(_angle_error(name, _chain32(name, "rotation", (src, gy)).d_theta), "angle")


def test_planted_dropped_corner_block_of_the_padding_adjoint():
    """On the first case's affine rows: the only one of the first / fourth / last cases whose sample points reach the corner
    blocks of the padding (a pure rotation of a centred crop never does; the fourth case has no padding, the last case's
    three rows all zoom in)."""
    name = FIRST
    c = ac.CASE_BY_NAME[name]
    r = ac.input_gradient_reference(name, "affine", True)
    d = r.f32.d_src.clone()
    d[:, :, 0, 0] -= r.f32.d_frame[:, :, :c.pad, :c.pad].sum(dim=(-1, -2))
    errs = ac.measure_input_gradient(d, r.f64.d_src)
    _caught(errs["corners"], "input:corners")
    assert errs["interior"] <= ac.budgets()["input:interior"] and errs["borders"] <= ac.budgets()["input:borders"]


def test_planted_channel_map_instead_of_its_inverse():
    name = FOURTH
    s = ac.setup(ac.CASE_BY_NAME[name], "rotation")
    inverse = torch.argsort(s.chan_map.long(), dim=1).to(torch.int32)
    assert not torch.equal(inverse, s.chan_map)
    d = _chain32(name, "rotation", ac.noise_inputs(name), chan_map=inverse).d_src
    errs = ac.measure_input_gradient(d, ac.input_gradient_reference(name, "rotation").f64.d_src)
    _caught(errs["interior"], "input:interior")
    _caught(errs["borders"], "input:borders")


def test_planted_flip_src_treated_as_flip_dst():
    """On the canonicalize D4 case, the one with FLIP_SRC (none of the first / fourth / last cases has flags)."""
    name = "canonicalize-d4"
    s = ac.setup(ac.CASE_BY_NAME[name], "rotation")
    assert (s.flags == ref.FLIP_SRC).any()
    wrong = torch.where(s.flags == ref.FLIP_SRC, torch.full_like(s.flags, ref.FLIP_DST), s.flags)
    d = _chain32(name, "rotation", ac.noise_inputs(name), flags=wrong).d_src
    _caught(ac.measure_input_gradient(d, ac.input_gradient_reference(name, "rotation").f64.d_src)["interior"], "input:interior")
    src, gy, _ = ac.smooth_inputs(name, "rotation")
    _caught(_angle_error(name, _chain32(name, "rotation", (src, gy), flags=wrong).d_theta), "angle")


def test_planted_crop_offset_top_and_left_exchanged():
    """On the off-centre crop, the one case whose top differs from its left."""
    name = "off-centre-crop"
    c = ac.CASE_BY_NAME[name]
    top, left = c.top_left
    assert top != left
    d = _chain32(name, "rotation", ac.noise_inputs(name), top_left=(left, top)).d_src
    _caught(ac.measure_input_gradient(d, ac.input_gradient_reference(name, "rotation").f64.d_src)["interior"], "input:interior")
    src, gy, _ = ac.smooth_inputs(name, "rotation")
    _caught(_angle_error(name, _chain32(name, "rotation", (src, gy), top_left=(left, top)).d_theta), "angle")
    for rows in ("rotation", "affine"):
        src, gy, _ = ac.smooth_inputs(name, rows)
        t = ac.transform_gradient_reference(name, rows)
        _caught(ac.measure_theta_gradient(_chain32(name, rows, (src, gy), top_left=(left, top)).d_theta, t.f64.d_theta), "theta")
