"""GPU: the n-body canonicalizer's frame chain on its fused kernels (eqa_nbody_frame_fwd / _bwd, eqa_rigid_rows_bwd) and the routes of
EuclideanGroupNBody under autograd.

Reference: autograd through the class's own op-by-op path in fp64 on the CPU.  Yardstick: the same path in fp32 on the CPU, taken at
run time and pooled over the cases (tests/nbody_frame_cases.py); a fused gradient may be at most FACTOR x that figure away, per
tensor, relative to the tensor's largest fp64 gradient -- the rule of tests/test_gpu_vndeepsets.py.  Frames have cond <= 20, so the
yardstick is a few fp32 ulps; the kernels compute in fp64 and round once, which leaves them half an ulp of the result.
Every figure is printed before it is asserted (-s shows them); with EQA_NBODY_FP64_LOG=<file> they are appended to that file.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import nbody_frame_cases as fc  # noqa: E402
import vndeepsets_cases as vc  # noqa: E402
import equiadapt_amd as ea  # noqa: E402
from equiadapt_amd import ops  # noqa: E402

DEV = "cuda"
FACTOR = 4.0
KEYS = ["rotation_matrix", "translation_vectors", "rotation_matrix_inverse"]
# incoming gradients present -> the weights of the linear functional sum(wR R) + sum(w1 cloc) + sum(w2 cvel)
BACKWARD_CASES = {"all": ("wR", "w1", "w2"), "only-gR": ("wR",), "only-gcloc": ("w1",), "rows-not-wanted": ("wR", "w1", "w2")}


def log(line):
    print(line)
    path = os.environ.get("EQA_NBODY_FP64_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def dev(d):
    return {k: t.to(DEV) for k, t in d.items()}


@pytest.fixture(scope="module")
def refs():
    """(M, case) -> (fp64 gradients, fp32 CPU relative errors); ("invert", M) likewise for x R + t; and the pooled fp32 figure."""
    table = {}
    for M in fc.SIZES:
        d = fc.inputs(M)
        for name, use in BACKWARD_CASES.items():
            rows = name != "rows-not-wanted"
            g64 = fc.frame_chain(ea.EuclideanGroupNBody, d, torch.float64, use, rows)
            g32 = fc.frame_chain(ea.EuclideanGroupNBody, d, torch.float32, use, rows)
            table[(M, name)] = (g64, {k: fc.rel_error(g32[k], g64[k]) for k in g64 if float(g64[k].abs().max()) > 0})
        R = ea.EuclideanGroupNBody(None).modified_gram_schmidt(d["v"].double())
        g64, g32 = fc.invert_chain(d, R, torch.float64), fc.invert_chain(d, R.float(), torch.float32)
        table[("invert", M)] = (g64, {k: fc.rel_error(g32[k], g64[k]) for k in g64})
    pooled = max(max(e.values()) for _, e in table.values())
    log(f"frame backward: fp32 CPU error pooled over {len(table)} cases {pooled:.3e}; budget {FACTOR * pooled:.3e}")
    return table, pooled


def check(label, got, g64, e32, pooled):
    for k, ref in g64.items():
        if float(ref.abs().max()) == 0:                          # the functional does not reach this input: an exact zero
            assert got[k] is not None and not got[k].any(), (label, k)
            continue
        err = fc.rel_error(got[k], ref)
        log(f"  {label} {k}: fp32 CPU {e32[k]:.3e}  fused {err:.3e}  ratio to pooled fp32 {err / pooled:.2f}")
        assert err <= FACTOR * pooled, (label, k)


# ------------------------------------------------------------------------------------------------------------ 1 forward bits
@pytest.mark.parametrize("M", fc.SIZES)
def test_one_launch_forward_gives_the_bits_of_the_three_launches(M):
    d = dev(fc.inputs(M))
    R, cloc, cvel = ops.nbody_frame_fwd(d["v"], d["t"], d["loc"], d["vel"])
    R3 = ops.modified_gram_schmidt(d["v"])
    assert torch.equal(R, R3)
    assert torch.equal(cloc, ops.rigid_rows(d["loc"], R3, d["t"], inverse=True))
    assert torch.equal(cvel, ops.rigid_rows(d["vel"], R3, None, inverse=True))


# ------------------------------------------------------------------------------------------------------ 2 backward vs fp64
@pytest.mark.parametrize("M", fc.SIZES)
def test_frame_backward_within_four_times_the_fp32_cpu_error(M, refs):
    table, pooled = refs
    d = dev(fc.inputs(M))
    R, _, _ = ops.nbody_frame_fwd(d["v"], d["t"], d["loc"], d["vel"])
    args = (d["v"], d["t"], d["loc"], d["vel"], R)

    gv, gt, gloc, gvel = ops.nbody_frame_bwd(*args, d["wR"], d["w1"], d["w2"])
    check(f"M={M} all", {"v": gv, "t": gt, "loc": gloc, "vel": gvel}, *table[(M, "all")], pooled)

    gv, gt, gloc, gvel = ops.nbody_frame_bwd(*args, None, d["w1"], None)
    check(f"M={M} only-gcloc", {"v": gv, "t": gt, "loc": gloc, "vel": gvel}, *table[(M, "only-gcloc")], pooled)

    gv, gt, gloc, gvel = ops.nbody_frame_bwd(*args, d["wR"], d["w1"], d["w2"], need=(True, True, False, False))
    assert gloc is None and gvel is None
    check(f"M={M} rows-not-wanted", {"v": gv, "t": gt}, *table[(M, "rows-not-wanted")], pooled)

    # only gR: the modified_gram_schmidt Function alone, through the class
    can = ea.EuclideanGroupNBody(None)
    v = d["v"].clone().requires_grad_(True)
    (can.modified_gram_schmidt(v) * d["wR"]).sum().backward()
    assert can.last_route == "fused-train"
    g64, e32 = table[(M, "only-gR")]
    check(f"M={M} only-gR", {"v": v.grad}, {"v": g64["v"]}, e32, pooled)


@pytest.mark.parametrize("M", fc.SIZES)
def test_rigid_rows_backward_within_four_times_the_fp32_cpu_error(M, refs):
    table, pooled = refs
    d = dev(fc.inputs(M))
    R = ops.modified_gram_schmidt(d["v"])
    gx, gR = ops.rigid_rows_bwd(d["loc"], R, d["w3"])
    check(f"M={M} invert", {"x": gx, "R": gR}, *table[("invert", M)], pooled)
    only_x, none = ops.rigid_rows_bwd(None, R, d["w3"], need=(True, False))
    assert none is None and torch.equal(only_x, gx)
    none, only_R = ops.rigid_rows_bwd(d["loc"], None, d["w3"], need=(False, True))
    assert none is None and torch.equal(only_R, gR)


# ------------------------------------------------------------------------------------------------------------------ 3 golden
@pytest.mark.parametrize("M", fc.GOLDEN_SIZES)
def test_golden_outputs_and_gradients_on_the_device(golden, M):
    """Per size, outputs and gradients each against 4 x the stored fp32 reference's largest distance from the stored fp64 reference
    among the tensors of that kind (per tensor, relative to the tensor's largest fp64 entry)."""
    case = golden("nbody_frame_grads.pt")["cases"][M]
    d = dict(case["fp32"]["inputs"])
    can, out, grads = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float32, DEV)
    assert can.last_route == "fused-train" and can.last_invert_route == "fused-train"
    for kind, got in (("outputs", out), ("grads", grads)):
        ref64, ref32 = case["fp64"][kind], case["fp32"][kind]
        stored = {k: fc.rel_error(ref32[k].reshape(ref64[k].shape), ref64[k]) for k in ref64}
        budget = FACTOR * max(stored.values())
        for k in ref64:
            err = fc.rel_error(got[k].reshape(ref64[k].shape), ref64[k])
            log(f"golden M={M} {kind} {k}: stored fp32 {stored[k]:.3e}  fused {err:.3e}  budget {budget:.3e}")
        for k in ref64:
            assert fc.rel_error(got[k].reshape(ref64[k].shape), ref64[k]) <= budget, (kind, k)


# ----------------------------------------------------------------------------------------------------------- 4 repeatability
def test_two_backward_launches_give_the_same_bits():
    d = dev(fc.inputs(1030))
    R, _, _ = ops.nbody_frame_fwd(d["v"], d["t"], d["loc"], d["vel"])
    a = ops.nbody_frame_bwd(d["v"], d["t"], d["loc"], d["vel"], R, d["wR"], d["w1"], d["w2"])
    b = ops.nbody_frame_bwd(d["v"], d["t"], d["loc"], d["vel"], R, d["wR"], d["w1"], d["w2"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, b = ops.rigid_rows_bwd(d["loc"], R, d["w3"]), ops.rigid_rows_bwd(d["loc"], R, d["w3"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------------------- 5 row isolation
def test_a_degenerate_row_stays_in_its_row():
    M = 257
    d = dev(fc.inputs(M))

    def both(v):
        fwd = ops.nbody_frame_fwd(v, d["t"], d["loc"], d["vel"])
        bwd = ops.nbody_frame_bwd(v, d["t"], d["loc"], d["vel"], fwd[0], d["wR"], d["w1"], d["w2"])
        inv = ops.rigid_rows_bwd(d["loc"], fwd[0], d["w3"])
        return [*fwd, *bwd, *inv]

    clean = both(d["v"])
    v = d["v"].clone()
    v[3, 0] = 0.0
    broken = both(v)
    assert not torch.isfinite(broken[3][3]).any()               # row 3 of gv
    others = torch.arange(M, device=DEV) != 3
    for a, b in zip(clean, broken):
        assert torch.isfinite(a).all()
        assert torch.equal(a[others], b[others])


# ---------------------------------------------------------------------------------------------------------------- 6 the class
def test_the_class_with_a_stand_in_network(monkeypatch, refs):
    _, pooled = refs
    M = 257
    d = fc.inputs(M)
    _, out64, g64 = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float64, "cpu", fc.SlicedParameter)
    _, _, g32 = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float32, "cpu", fc.SlicedParameter)
    can, out, grads = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float32, DEV, fc.SlicedParameter)
    assert can.last_route == "fused-train", can.last_route
    assert can.last_invert_route == "fused-train", can.last_invert_route
    el = can.canonicalization_info_dict["group_element"]
    assert list(el) == KEYS
    assert torch.equal(el["rotation_matrix_inverse"], el["rotation_matrix"].transpose(1, 2))
    assert el["rotation_matrix"].requires_grad and el["translation_vectors"].shape == (M, 3)
    for k in ("out", "loc", "vel"):
        err = fc.rel_error(grads[k], g64[k])
        log(f"class M={M} {k}: fp32 CPU {fc.rel_error(g32[k], g64[k]):.3e}  fused {err:.3e}  ratio to pooled fp32 {err / pooled:.2f}")
        assert err <= FACTOR * pooled, k

    # a loss on the inverse frame reaches gR through autograd's transpose
    net = fc.SlicedParameter(d["v"], d["t"]).to(DEV)
    can2 = ea.EuclideanGroupNBody(net)
    fc.run(can2, d["loc"].to(DEV), d["vel"].to(DEV))
    wR = d["wR"].to(DEV)
    (can2.canonicalization_info_dict["group_element"]["rotation_matrix_inverse"] * wR).sum().backward()
    expect = ops.nbody_frame_bwd(net.out.detach()[:, :, :3], None, None, None, None, wR.transpose(1, 2), None, None,
                                 need=(True, False, False, False))[0]
    assert torch.equal(net.out.grad[:, :, :3], expect) and not net.out.grad[:, :, 3].any()

    with torch.no_grad():
        cloc, cvel = fc.run(can, d["loc"].to(DEV), d["vel"].to(DEV))
        assert can.last_route == "fused-inference"
        inverted = can.invert_canonicalization(0.5 * cloc + cvel)
        assert can.last_invert_route == "fused-inference"
    assert torch.equal(cloc, out["cloc"]) and torch.equal(cvel, out["cvel"]) and torch.equal(inverted, out["inverted"])
    assert torch.equal(can.canonicalization_info_dict["group_element"]["rotation_matrix"], out["R"])

    monkeypatch.setenv("EQA_NBODY_FRAME_KERNEL", "0")
    can3, out3, _ = fc.golden_chain(ea.EuclideanGroupNBody, d, torch.float32, DEV, fc.SlicedParameter)
    monkeypatch.delenv("EQA_NBODY_FRAME_KERNEL")
    assert can3.last_route.startswith("plain") and "EQA_NBODY_FRAME_KERNEL=0" in can3.last_route
    assert can3.last_invert_route.startswith("plain")
    assert (out3["cloc"].double().cpu() - out64["cloc"]).abs().max() <= 1e-4

    class Own(ea.EuclideanGroupNBody):
        def modified_gram_schmidt(self, vectors):
            return super().modified_gram_schmidt(vectors)

    can4, out4, g4 = fc.golden_chain(Own, d, torch.float32, DEV, fc.SlicedParameter)
    assert can4.last_route.startswith("plain"), can4.last_route
    assert list(can4.canonicalization_info_dict["group_element"]) == KEYS
    assert fc.rel_error(g4["out"], g64["out"]) <= FACTOR * pooled


# --------------------------------------------------------------------------------------------------- 7 end to end, VNDeepSets
E2E = dict(train=True, dropout=0.0, canon_feature="pv", canon_translation=True)
E2E_CASES = [
    vc.case("pv-S1", 1, seed=0, **E2E),
    vc.case("pv-S6", 6, seed=1, **E2E),
    vc.case("pv-S67", 67, seed=2, **E2E),
    vc.case("pvac-leaky-S67", 67, seed=3, **dict(E2E, nonlinearity="leakyrelu", canon_feature="pvac")),
]


def e2e_gradients(c, dtype, device, keep):
    net, d = vc.build(c, dtype, device)
    M = 5 * c["S"]
    g = torch.Generator().manual_seed(3000 + c["seed"])
    w1, w2, w3 = (torch.randn(M, 3, generator=g).to(device=device, dtype=dtype) for _ in range(3))
    can = ea.EuclideanGroupNBody(net)
    nodes = torch.ones(M, 1, dtype=dtype, device=device)
    cloc, cvel = can(nodes, loc=d["loc"], edges=d["edges"], vel=d["vel"], edge_attr=None, charges=d["charges"])
    weight = keep.to(device=device, dtype=dtype).repeat_interleave(5)
    loss, _ = fc.golden_loss(can, cloc, cvel, w1, w2, w3, weight)
    loss.backward()
    return net, can, {n: p.grad.detach().clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize("c", E2E_CASES, ids=[c["name"] for c in E2E_CASES])
def test_canonicalizer_trains_end_to_end_with_vndeepsets(c):
    keep = vc.kink_free_systems(c)
    dropped = int((~keep).sum())
    log(f"end to end {c['name']}: {dropped} of {c['S']} systems within {vc.KINK_COS} of a kink carry no weight")
    assert dropped <= vc.MAX_DROPPED * c["S"]
    _, _, g64 = e2e_gradients(c, torch.float64, "cpu", keep)
    _, _, g32 = e2e_gradients(c, torch.float32, "cpu", keep)
    own = max(fc.rel_error(g32[k], g64[k]) for k in g64)
    net, can, grads = e2e_gradients(c, torch.float32, DEV, keep)
    assert net.last_route == "fused-train", net.last_route
    assert can.last_route == "fused-train", can.last_route
    assert can.last_invert_route == "fused-train", can.last_invert_route
    errs = {k: fc.rel_error(grads[k], g64[k]) for k in g64}
    log(f"end to end {c['name']}: fp32 CPU {own:.3e}  fused worst tensor {max(errs.values()):.3e}  ratio {max(errs.values()) / own:.2f}")
    for k, err in errs.items():
        assert err <= FACTOR * own, (k, err, own)
