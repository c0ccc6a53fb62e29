"""CPU: the references, measures and budgets of tests/winograd_backward_cases.py, which tests/test_gpu_winograd_backward_fp64.py
holds the Winograd convolution's gradient kernels to.

1. The chain IS the gradient: evaluated in fp64 it reproduces autograd's fp64 gradients of F.conv2d to 1e-12 on every case and
   both tile sizes -- layout, signs, padding, flip and transpose of the bank, fold-back.
2. Torch's fp32 evaluation of the two transforms stays inside the a-priori bound that the kernels are held to.
3. The budgets have teeth: each pooled budget is at most 1e-4 (30 times under the 3e-3 of the network-level test).
4. Planted errors: a result with ONE defect of the kind a kernel could have must exceed its budget (or the a-priori bound).
   A check that cannot fail holds nothing.
"""
import pytest
import torch

import winograd_backward_cases as wc

RUNS = [(c.name, m) for c in wc.CASES for m in wc.tiles_of(c)]
IDS = [f"{n}-m{m}" for n, m in RUNS]


def test_every_case_runs_both_tile_sizes():
    assert all(wc.tiles_of(c) == (2, 4) for c in wc.CASES)


def test_cases_reach_what_they_are_there_for():
    """The strip, work-order, channel-block and chunk arithmetic of the cases, from the host code's own formulas
    (wc.launch_plan restates launch_wino_input; wc.chunk_sizes the loop of winograd.conv5x5 / filter_grad)."""
    plan = lambda name, m, padded: wc.launch_plan(  # noqa: E731
        wc.CASE_BY_NAME[name].B, wc.CASE_BY_NAME[name].H + (4 if padded else 0), wc.CASE_BY_NAME[name].W + (4 if padded else 0),
        wc.CASE_BY_NAME[name].Cout if padded else wc.CASE_BY_NAME[name].Cin, m)
    # F(4x4) with strips, plain: x 32 x 40, TX = 9, a shorter last strip
    p = plan("strips", 4, False)
    assert (p["TX"], p["strips"]) == (9, (5, 4))
    # ... its own dy (28 x 36) gives the padded form even strips and work counts on the multiples of 8:
    assert plan("strips", 4, True)["strips"] == (5, 5) and plan("strips", 4, True)["nwork"] == 48
    assert plan("strips", 2, True)["strips"] == (4,) * 5 and plan("strips", 2, True)["nwork"] == 240
    # ... which is what "strips-padded" (dy 32 x 40) is there for: uneven strips, work counts off the multiples of 8
    p = plan("strips-padded", 4, True)
    assert (p["TY"], p["TX"], p["strips"], p["nwork"]) == (9, 11, (6, 5), 54) and p["nwork"] % 8
    p = plan("strips-padded", 2, True)
    assert (p["TY"], p["TX"], p["strips"], p["nwork"]) == (18, 22, (5, 5, 5, 5, 2), 270) and p["nwork"] % 8
    assert plan("strips-padded", 4, False)["strips"] == (5, 5) and plan("strips-padded", 2, False)["strips"] == (4,) * 5
    # non-square, one strip per tile row (but two even ones in the padded m = 2 form), work counts off the multiples of 8
    for m in (2, 4):
        for padded in (False, True):
            p = plan("off-32", m, padded)
            assert p["strips"] == ((4, 4) if (m, padded) == (2, True) else (p["TX"],)) and p["TY"] != p["TX"] and p["nwork"] % 8
    # a second, partly filled channel block on both sides
    for m in (2, 4):
        assert (plan("wide", m, False)["channel_blocks"], plan("wide", m, False)["last_block_lanes"]) == (2, 32)
        assert (plan("wide", m, True)["channel_blocks"], plan("wide", m, True)["last_block_lanes"]) == (2, 64)
    assert all(wc.launch_plan(c.B, c.H, c.W, c.Cin, 2)["channel_blocks"] == 1 for c in wc.CASES if c.name != "wide")
    # chunks
    c = wc.CASE_BY_NAME["chunks"]
    assert wc.chunk_sizes(c.B, 2, 2) == (2, 2, 2, 2, 1) and wc.chunk_sizes(c.B, 4, 2) == (8, 1)
    assert wc.chunk_sizes(c.B, 2, 64) == (9,) and wc.chunk_sizes(c.B, 4, 64) == (9,)
    # the two GEMM routes: eqa_plane_gemm takes channel counts on the 32-multiples only; 48 is the one that is off them
    assert [(c.Cin % 32, c.Cout % 32) for c in wc.CASES] == [(0, 16), (0, 0), (0, 0), (0, 0), (0, 0)]


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_fp64_chain_reproduces_autograd(name, m):
    want, got = wc.reference(name), wc.chain_results(name, m, fp64=True)
    assert wc.measure(got.y, want.y) <= 1e-12
    assert wc.measure(got.d_bank, want.d_bank) <= 1e-12
    errs = wc.measure_input_gradient(got.d_x, want.d_x)
    assert max(errs.values()) <= 1e-12, errs


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_fp32_transforms_stay_inside_the_a_priori_bound(name, m):
    """Torch's fp32 einsum of A dY A^T and B^T d B (padded and plain) against their fp64 evaluation: inside the bound, and not
    by so much that the bound would hold nothing (above 1 / 1000 of it)."""
    x, _, dy = wc.inputs(name)
    for got, ref in ((wc.output_adjoint(dy, m), wc.adjoint_reference(name, m)),
                     (wc.input_transform(dy, m, 4), wc.padded_input_reference(name, m)),
                     (wc.input_transform(x, m), wc.plain_input_reference(name, m))):
        assert got.dtype == torch.float32
        r = wc.measure_transform(got, ref)
        assert 1e-3 <= r <= 1.0, (name, m, r)


def test_measure_demands_exact_zeros_where_the_bound_is_zero():
    """The a-priori bound is zero where every tap of an entry lies in the padding (pad = 4 leaves no such entry; a map of zeros
    in one channel does); the measure then demands an exact zero."""
    dy = wc.inputs("off-32")[2].double().clone()
    dy[:, 0] = 0.0
    ref = wc.TransformReference(wc.input_transform(dy, 2, 4), wc.TRANSFORM_GAMMA * wc.input_transform(dy, 2, 4, absolute=True))
    assert (ref.bound == 0).any() and (ref.want[ref.bound == 0] == 0).all()
    got = ref.want.clone()
    assert wc.measure_transform(got, ref) == 0.0
    got[ref.bound == 0] = 1e-30
    assert wc.measure_transform(got, ref) == float("inf")


def test_budgets_have_teeth():
    """Measured here: d_bank 4.4e-6 ... 1.8e-5, d_x 3.2e-6 ... 7.1e-6 for the fp32 CPU chain, so budgets of about 7e-5 and 3e-5.
    If a case pushes one above 1e-4, the case is to change, not this cap."""
    b = wc.budgets()
    assert set(b) == set(wc.QUANTITIES)
    for q, v in b.items():
        assert 0.0 < v <= 1e-4, (q, v)
    # the chain passes its own check, case by case, and its forward is inside the forward test's bound
    for key, v in wc.cpu_chain_errors().items():
        assert v <= (b[key[0]] / wc.M_BUDGET if key[0] in b else wc.FORWARD_BOUND), (key, v)


# ---- planted errors ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_planted_dropped_border_tap(name, m):
    """d_x whose border pixels lack the contribution of ONE of the 25 filter taps (a tap that the padding logic drops); the
    interior is untouched and stays inside its budget."""
    x, bank, dy = (t.double() for t in wc.inputs(name))
    want = wc.reference(name).d_x
    one_tap = torch.zeros_like(bank)
    one_tap[:, :, 0, 0] = bank[:, :, 0, 0]
    contribution = torch.nn.grad.conv2d_input(x.shape, one_tap, dy)
    wrong = want.clone()
    b = wc.border_mask(*want.shape[-2:])
    wrong[..., b] -= contribution[..., b]
    errs = wc.measure_input_gradient(wrong, want)
    assert errs["d_x:border"] > wc.budgets()["d_x:border"], errs
    assert errs["d_x:interior"] == 0.0
    # and a single zeroed border entry of the gradient (the largest one of the first image's first channel)
    wrong = want.clone()
    flat = torch.where(b, want[0, 0].abs(), torch.zeros((), dtype=want.dtype)).argmax().item()
    wrong[0, 0, flat // want.shape[-1], flat % want.shape[-1]] = 0.0
    assert wc.measure_input_gradient(wrong, want)["d_x:border"] > wc.budgets()["d_x:border"]


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_planted_tile_column_shifted(name, m):
    """One tile column taken from m pixels to the right: in d_x (the output transform's tile index), and in both transforms'
    (tiles, P, C) results (the strip walk's window)."""
    c = wc.CASE_BY_NAME[name]
    want = wc.reference(name).d_x
    tx = (c.W // m - 1) // 2
    wrong = want.clone()
    wrong[..., m * tx:m * tx + m] = want[..., m * tx + m:m * tx + 2 * m]
    errs = wc.measure_input_gradient(wrong, want)
    assert errs["d_x:interior"] > wc.budgets()["d_x:interior"] and errs["d_x:border"] > wc.budgets()["d_x:border"], errs
    for ref, TX in ((wc.adjoint_reference(name, m), (c.W - 4) // m), (wc.padded_input_reference(name, m), c.W // m)):
        t = ref.want.reshape(c.B, -1, TX, *ref.want.shape[1:])
        wrong = t.clone()
        wrong[:, :, (TX - 1) // 2] = t[:, :, (TX - 1) // 2 + 1]
        assert wc.measure_transform(wrong.reshape(ref.want.shape), ref) > 1e3


@pytest.mark.parametrize("name,m", RUNS, ids=IDS)
def test_planted_transform_coefficient(name, m):
    """One coefficient of a transform off by one part in a thousand (5.25 -> 5.255 is 1e-3): far outside the a-priori bound."""
    ref = wc.adjoint_reference(name, m)
    wrong = ref.want.clone()
    wrong[:, 1] *= 1.001
    assert wc.measure_transform(wrong, ref) > 10.0


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_planted_bank_gradient_transposed(name):
    """d_bank with its last two axes (the filter's rows and columns) exchanged."""
    want = wc.reference(name).d_bank
    assert wc.measure(want.transpose(-1, -2), want) > wc.budgets()["d_bank"]
    assert wc.measure(want.transpose(-1, -2), want) > 0.1
