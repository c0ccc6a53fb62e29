"""GPU: every backward kernel of the group action (and the forward on general affine rows) against the fp64 reference of
oracle/action_fp64.py, each kernel on its own.

``ops.group_action_bwd`` is called directly with theta tables of this file's own angles, once in the default state and once
under ``eqa_set_option(0, 1)``; both are held to the SAME fp64 reference, so no kernel is judged by another kernel:

    default                                            eqa_set_option(0, 1)
    staged angle kernel (group_action_angle_kernel)    group_action_bwd_kernel<1, false>, <1, true>
    gather adjoint (un-padded)                         atomic scatter <0, true>, <1, true>, <2, true>
    frame gather + eqa_fold_edge_pad (padded)          (the same scatter, through the clamped offsets)
    group_action_bwd_kernel<2, false>                  group_action_bwd_kernel<2, false>, <2, true>

Cases, inputs, measures and budgets: tests/action_backward_cases.py.  The budgets are M = 4 times the error of torch's fp32 CPU
evaluation of the same chain, pooled over the cases and computed at run time; nothing is taken from the kernels.  The inputs
keep the angle and theta gradients away from the kinks of the bilinear interpolant (see there), which is what lets the bound be
4 times an fp32 rounding error instead of the 2e-3 / 35 % of tests/test_gpu_backward.py; right angles stay with those tests.

Measured on an MI355X (profiles/r11/backward_fp64.txt lists every case; findings in profiles/r11/README.md), kernel error /
fp32 CPU error: input gradient 0.96 - 1.07 in every region and kernel, angle gradient 0.05 - 0.57, theta gradient 0.11 - 0.65,
forward 1.000.  The bound is 4.

With EQA_BACKWARD_FP64_LOG=<file> every measured figure (fp32 CPU error, kernel error, their ratio, share of zeroed pixels) is
appended to that file.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import action_backward_cases as ac  # noqa: E402

STATES = ("default", "forced-direct")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(params=STATES)
def state(request):
    """Run the test body under eqa_set_option(0, value), restored afterwards."""
    from equiadapt_amd import _lib

    lib = _lib.load()
    before = lib.eqa_get_option(0)
    lib.eqa_set_option(0, 1 if request.param == "forced-direct" else 0)
    try:
        yield request.param
    finally:
        lib.eqa_set_option(0, before)


def _on(dev, s: ac.Setup):
    opt = lambda t: None if t is None else t.to(dev)  # noqa: E731
    return s.gidx.to(dev), s.theta.to(dev), opt(s.flags), opt(s.chan_map)


def _bwd(dev, s: ac.Setup, src, gy, want_src, want_angle, want_theta=False):
    from equiadapt_amd import ops

    c = s.case
    gidx, theta, flags, cmap = _on(dev, s)
    return ops.group_action_bwd(src.to(dev), gy.to(dev), gidx, theta, flags, cmap, c.pad, c.top_left, want_src, want_angle,
                                want_theta)


def _record(quantity, case, rows, state, kernels, cpu_err, got_err, zeroed=None):
    """Print the figure (shown when the assertion below it fails) and append it to the log file if one is asked for."""
    ratio = got_err / cpu_err if cpu_err > 0 else (0.0 if got_err == 0 else float("inf"))
    line = (f"{quantity:15s} {case:20s} {rows:9s} {state:13s} {kernels:34s} fp32-cpu {cpu_err:9.3e}  kernel {got_err:9.3e}  "
            f"ratio {ratio:7.3f}  budget {ac.budgets()[quantity]:9.3e}" + (f"  zeroed {100 * zeroed:5.2f} %" if zeroed is not None else ""))
    print(line)
    path = os.environ.get("EQA_BACKWARD_FP64_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check_input_gradient(got, case, rows, state, kernels):
    r = ac.input_gradient_reference(case.name, rows)
    errs = ac.measure_input_gradient(got, r.f64.d_src)
    for region, v in errs.items():
        _record("input:" + region, case.name, rows, state, kernels, ac.cpu_chain_errors()[("input:" + region, case.name, rows)], v)
    for region, v in errs.items():
        assert v <= ac.budgets()["input:" + region], (case.name, rows, state, kernels, region, v, ac.budgets()["input:" + region])


INPUT_RUNS = [(c.name, rows) for c in ac.CASES for rows in ac.input_gradient_row_sets(c)]


@pytest.mark.parametrize("name,rows", INPUT_RUNS, ids=[f"{n}-{r}" for n, r in INPUT_RUNS])
def test_input_gradient_matches_fp64(dev, state, name, rows):
    """dL/dsrc on white noise with a full output gradient.  Default: the gather adjoint (un-padded) or the frame gather and the
    fold of the padding's strips and corners (padded).  Forced: the atomic scatter, alone (<0, true>), next to the angle
    gradient (<1, true>) and, for the per-sample rows, next to the theta gradient (<2, true>)."""
    case = ac.CASE_BY_NAME[name]
    s = ac.setup(case, rows)
    src, gy = ac.noise_inputs(name)
    forced = state == "forced-direct"
    g, _ = _bwd(dev, s, src, gy, True, False)
    _check_input_gradient(g, case, rows, state, "scatter<0,true>" if forced else ("frame gather + fold" if case.pad else "gather adjoint"))
    if rows != "affine":      # (the angle kernels take a rotation; their own output is judged in the angle test)
        g, _ = _bwd(dev, s, src, gy, True, True)
        _check_input_gradient(g, case, rows, state, "scatter<1,true>" if forced else "(same) + angle kernel")
    if case.theta_case:
        g, _ = _bwd(dev, s, src, gy, True, False, want_theta=True)
        _check_input_gradient(g, case, rows, state, "scatter<2,true>" if forced else "(same) + bwd<2,false>")


@pytest.mark.parametrize("name", [c.name for c in ac.CASES])
def test_angle_gradient_matches_fp64(dev, state, name):
    """dL/d angle (per degree) on smooth images, output gradient zeroed at the kinks.  Default: the staged angle kernel (with the
    in-kernel direct path where a window exceeds 47 rows).  Forced: group_action_bwd_kernel<1, false> and, together with the
    input gradient, <1, true>."""
    case = ac.CASE_BY_NAME[name]
    zeroed = ac.check_inputs_are_unambiguous(name, "rotation")
    s = ac.setup(case, "rotation")
    src, gy, _ = ac.smooth_inputs(name, "rotation")
    want = ac.angle_gradient(ac.transform_gradient_reference(name, "rotation").f64.d_theta, ac.angle_jacobian(name))
    forced = state == "forced-direct"
    results = []
    for want_src, kernels in ((False, "bwd<1,false>" if forced else "staged angle kernel"),
                              (True, "bwd<1,true>" if forced else "staged angle kernel (+ input)")):
        _, got = _bwd(dev, s, src, gy, want_src, True)
        assert got.shape == (case.B,)
        err = ac.measure_per_image(got, want)
        _record("angle", name, "rotation", state, kernels, ac.cpu_chain_errors()[("angle", name)], err, zeroed)
        results.append((kernels, err))
    for kernels, err in results:
        assert err <= ac.budgets()["angle"], (name, state, kernels, err, ac.budgets()["angle"])


THETA_RUNS = [(c.name, rows) for c in ac.THETA_CASES for rows in ("rotation", "affine")]


@pytest.mark.parametrize("name,rows", THETA_RUNS, ids=[f"{n}-{r}" for n, r in THETA_RUNS])
def test_theta_gradient_matches_fp64(dev, state, name, rows):
    """dL/dtheta, all six components per output image, for per-sample rows: rotations, and general affine rows that move the
    six components independently.  group_action_bwd_kernel<2, false>; forced and with the input gradient, <2, true>."""
    case = ac.CASE_BY_NAME[name]
    zeroed = ac.check_inputs_are_unambiguous(name, rows)
    s = ac.setup(case, rows)
    src, gy, _ = ac.smooth_inputs(name, rows)
    want = ac.transform_gradient_reference(name, rows).f64.d_theta
    forced = state == "forced-direct"
    results = []
    for want_src, kernels in ((False, "bwd<2,false>"), (True, "bwd<2,true>" if forced else "bwd<2,false> (+ input)")):
        _, got = _bwd(dev, s, src, gy, want_src, False, want_theta=True)
        assert got.shape == (case.B, 6)
        err = ac.measure_theta_gradient(got, want)
        _record("theta", name, rows, state, kernels, ac.cpu_chain_errors()[("theta", name, rows)], err, zeroed)
        results.append((kernels, err))
    for kernels, err in results:
        assert err <= ac.budgets()["theta"], (name, rows, state, kernels, err, ac.budgets()["theta"])


@pytest.mark.parametrize("name", [c.name for c in ac.THETA_CASES])
def test_forward_on_affine_rows_matches_fp64(dev, state, name):
    """The forward on the general affine rows: scales above 1 make a tile's window exceed the staged 47 x 47 box, which takes the
    direct path INSIDE the forward kernel (forced: every tile takes it)."""
    from equiadapt_amd import ops

    case = ac.CASE_BY_NAME[name]
    s = ac.setup(case, "affine")
    src, _, _ = ac.smooth_inputs(name, "affine")
    gidx, theta, flags, cmap = _on(dev, s)
    got = ops.group_action(src.to(dev), gidx, theta, flags, cmap, case.pad, case.out_hw, case.top_left)
    err = ac.measure_forward(got, ac.transform_gradient_reference(name, "affine").f64.out)
    _record("forward", name, "affine", state, "group_action_kernel", ac.cpu_chain_errors()[("forward", name)], err)
    assert err <= ac.budgets()["forward"], (name, state, err, ac.budgets()["forward"])
