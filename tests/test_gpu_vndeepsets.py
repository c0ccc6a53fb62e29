"""GPU: the fused route of VNDeepSets (eqa_nbody_adjacency, eqa_vndeepsets_fwd / _train_fwd / _bwd) against the fp64 CPU plain route.

Budget (tests/vndeepsets_cases.py): the fused route's error may be at most 4 x the error of torch's fp32 CPU plain route against the
same fp64 result, that figure computed here and pooled over the cases.  Outputs are judged relative to max(1, max |fp64 output|) of
the case, gradients per parameter tensor relative to that tensor's largest fp64 gradient, against the pooled figure and
against 4 x the case's own fp32 CPU figure (the largest over its tensors), whichever is smaller.  Every figure is printed before it is
asserted (-s shows them); with EQA_NBODY_FP64_LOG=<file> they are appended to that file.

Measured on one MI355X (profiles/r16/vndeepsets_fp64.txt): see the table in profiles/r16/README.md.
"""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import vndeepsets_cases as vc  # noqa: E402
import equiadapt_amd as ea  # noqa: E402
from equiadapt_amd.nbody import complete_graph_edges, graph  # noqa: E402
from equiadapt_amd.nbody.canonicalization_networks import VNDeepSets  # noqa: E402

DEV = "cuda"
FACTOR = 4.0


def log(line):
    print(line)
    path = os.environ.get("EQA_NBODY_FP64_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def out_error(out, ref):
    scale = max(1.0, float(ref[0].abs().max()))
    return max(float((out[0].double().cpu() - ref[0]).abs().max()), float((out[1].double().cpu() - ref[1]).abs().max())) / scale


@pytest.fixture(scope="module")
def forward_refs():
    """name -> (fp64 outputs, fp32 CPU error); and the pooled fp32 figure."""
    refs = {}
    for c in vc.FORWARD_CASES:
        n64, d64 = vc.build(c, torch.float64, "cpu")
        n32, d32 = vc.build(c, torch.float32, "cpu")
        with torch.no_grad():
            ref = vc.forward(n64, d64)
            e32 = out_error(vc.forward(n32, d32), ref)
        refs[c["name"]] = (ref, e32)
    pooled = max(e for _, e in refs.values())
    log(f"forward: fp32 CPU error pooled over {len(refs)} cases {pooled:.3e}; budget {FACTOR * pooled:.3e}")
    return refs, pooled


@pytest.fixture(scope="module")
def backward_refs():
    """name -> (system weights, fp64 gradients, fp32 CPU relative errors per tensor); and the pooled fp32 figure."""
    refs = {}
    for c in vc.BACKWARD_CASES:
        keep = vc.kink_free_systems(c)
        n64, d64 = vc.build(c, torch.float64, "cpu")
        n32, d32 = vc.build(c, torch.float32, "cpu")
        g64 = vc.gradients(n64, d64, keep)
        g32 = vc.gradients(n32, d32, keep)
        e32 = {k: float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64}
        refs[c["name"]] = (keep, g64, e32)
    pooled = max(max(e.values()) for _, _, e in refs.values())
    log(f"backward: fp32 CPU error pooled over {len(refs)} cases {pooled:.3e}; budget {FACTOR * pooled:.3e}")
    return refs, pooled


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", vc.FORWARD_CASES, ids=[c["name"] for c in vc.FORWARD_CASES])
def test_fused_forward_within_four_times_the_fp32_cpu_error(c, forward_refs):
    refs, pooled = forward_refs
    ref, e32 = refs[c["name"]]
    net, d = vc.build(c, torch.float32, DEV)
    with torch.no_grad():
        out = vc.forward(net, d)
    assert net.last_route == "fused-inference", net.last_route
    assert out[0].shape == ref[0].shape and out[1].shape == ref[1].shape
    err = out_error(out, ref)
    log(f"forward {c['name']}: fp32 CPU {e32:.3e}  fused {err:.3e}  ratio to pooled fp32 {err / pooled:.2f}")
    assert err <= FACTOR * pooled


@pytest.mark.parametrize("name", ["default", "pvac_leakyrelu_sum", "pv_softplus", "ring"])
def test_golden_cases_on_the_device(golden, name, forward_refs):
    _, pooled = forward_refs
    case = golden("vndeepsets.pt")["cases"][name]
    hp = types.SimpleNamespace(**case["hyperparams"])
    net64 = VNDeepSets(hp, device="cpu").double().eval()
    net64.load_state_dict(case["state"], strict=True)
    with torch.no_grad():
        ref = net64(None, case["loc"].double(), case["edges"], case["vel"].double(), None, case["charges"].double())
    net = VNDeepSets(hp, device=DEV).to(DEV).eval()
    net.load_state_dict(case["state"], strict=True)
    with torch.no_grad():
        out = net(None, case["loc"].to(DEV), [e.to(DEV) for e in case["edges"]], case["vel"].to(DEV), None, case["charges"].to(DEV))
    assert net.last_route == "fused-inference"
    err = out_error(out, ref)
    stored = out_error((case["rotation_vectors"], case["translation_vectors"]), ref)
    log(f"golden {name}: stored reference output {stored:.3e} from fp64, fused {err:.3e}")
    assert err <= FACTOR * pooled
    # and next to the stored reference output itself: both are within their own distance of the fp64 result
    assert out_error(out, (case["rotation_vectors"].double(), case["translation_vectors"].double())) <= FACTOR * pooled + stored


def test_golden_prediction_mode_on_the_device(golden, forward_refs):
    """out_dim = 1 takes the plain route on the device as well; its per-node output against the stored reference output."""
    _, pooled = forward_refs
    case = golden("vndeepsets.pt")["cases"]["prediction_mode"]
    hp = types.SimpleNamespace(**case["hyperparams"])
    net64 = VNDeepSets(hp, device="cpu").double().eval()
    net64.load_state_dict(case["state"], strict=True)
    with torch.no_grad():
        ref = net64(None, case["loc"].double(), case["edges"], case["vel"].double(), None, case["charges"].double())
    net = VNDeepSets(hp, device=DEV).to(DEV).eval()
    net.load_state_dict(case["state"], strict=True)
    with torch.no_grad():
        out = net(None, case["loc"].to(DEV), [e.to(DEV) for e in case["edges"]], case["vel"].to(DEV), None, case["charges"].to(DEV))
    assert net.last_route.startswith("plain: prediction"), net.last_route
    assert out.shape == case["prediction"].shape
    scale = max(1.0, float(ref.abs().max()))
    err = float((out.double().cpu() - ref).abs().max()) / scale
    stored = float((case["prediction"].double() - ref).abs().max()) / scale
    log(f"golden prediction_mode: stored reference output {stored:.3e} from fp64, plain route on the device {err:.3e}")
    assert err <= FACTOR * pooled
    assert float((out.cpu() - case["prediction"]).abs().max()) / scale <= FACTOR * pooled + stored


# --------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("c", vc.BACKWARD_CASES, ids=[c["name"] for c in vc.BACKWARD_CASES])
def test_fused_gradients_within_four_times_the_fp32_cpu_error(c, backward_refs):
    refs, pooled = backward_refs
    keep, g64, e32 = refs[c["name"]]
    dropped = int((~keep).sum())
    log(f"backward {c['name']}: {dropped} of {c['S']} systems within {vc.KINK_COS} of a kink carry no weight")
    assert dropped <= vc.MAX_DROPPED * c["S"]
    net, d = vc.build(c, torch.float32, DEV)
    grads = vc.gradients(net, d, keep)
    assert net.last_route == "fused-train", net.last_route
    worst = 0.0
    for k in g64:
        err = float((grads[k].double().cpu() - g64[k]).abs().max() / g64[k].abs().max())
        worst = max(worst, err)
        log(f"  {k}: fp32 CPU {e32[k]:.3e}  fused {err:.3e}")
    log(f"backward {c['name']}: worst tensor {worst:.3e}  ratio to pooled fp32 {worst / pooled:.2f}"
        f"  to the case's own fp32 {worst / max(e32.values()):.2f}")
    own = max(e32.values())
    for k in g64:
        err = float((grads[k].double().cpu() - g64[k]).abs().max() / g64[k].abs().max())
        assert err <= FACTOR * pooled, k
        assert err <= FACTOR * own, (k, "the case's own fp32 CPU figure", own)


def test_two_launches_give_the_same_bits():
    c = vc.BACKWARD_CASES[1]                                    # the default configuration, S = 67, training with a mask
    net, d = vc.build(c, torch.float32, DEV)
    keep = torch.ones(c["S"], dtype=torch.bool)
    with torch.no_grad():
        a, b = vc.forward(net, d), vc.forward(net, d)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    g1, g2 = vc.gradients(net, d, keep), vc.gradients(net, d, keep)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    net.eval()
    d["mask"] = None
    with torch.no_grad():
        a, b = vc.forward(net, d), vc.forward(net, d)
    assert net.last_route == "fused-inference"
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------------- routes
def _route(c, dtype=torch.float32, grad=False, prepare=None):
    net, d = vc.build(c, dtype, DEV)
    if prepare:
        prepare(net, d)
    with torch.set_grad_enabled(grad):
        out = vc.forward(net, d)
    return net, d, out


def test_routes(monkeypatch):
    base = vc.case("routes", 5, canon_feature="pv")
    assert _route(base)[0].last_route == "fused-inference"
    assert _route(base, grad=True)[0].last_route == "fused-train"
    assert _route(vc.case("sp", 5, nonlinearity="softplus"))[0].last_route == "fused-inference"
    plain = {
        "fp64": _route(base, dtype=torch.float64)[0],
        "prediction mode": _route(vc.case("pm", 5, out_dim=1))[0],
        "hidden 33": _route(vc.case("h33", 5, hidden_dim=33))[0],
        "softplus under autograd": _route(vc.case("sp", 5, nonlinearity="softplus"), grad=True)[0],
        "input requires grad": _route(base, grad=True, prepare=lambda net, d: d["loc"].requires_grad_(True))[0],
    }
    monkeypatch.setenv("EQA_NBODY_KERNEL", "0")
    plain["switch"] = _route(base)[0]
    monkeypatch.delenv("EQA_NBODY_KERNEL")
    for why, net in plain.items():
        assert net.last_route.startswith("plain"), (why, net.last_route)
    assert "EQA_NBODY_KERNEL=0" in plain["switch"].last_route


def test_cross_system_edge_takes_the_plain_route_and_is_right():
    c = vc.case("cross", 5, canon_feature="pv")

    def add_cross_edge(net, d):
        d["edges"] = [torch.cat([d["edges"][0], torch.tensor([2], device=DEV)]), torch.cat([d["edges"][1], torch.tensor([7], device=DEV)])]

    net, d, out = _route(c, prepare=add_cross_edge)
    assert net.last_route.startswith("plain: edges"), net.last_route
    n64, d64 = vc.build(c, torch.float64, "cpu")
    d64["edges"] = [e.cpu() for e in d["edges"]]
    with torch.no_grad():
        ref = vc.forward(n64, d64)
    assert out_error(out, ref) <= 1e-5


def test_complete_graph_edges_validate_once(monkeypatch):
    S = 9
    c = vc.case("once", S)
    net, d = vc.build(c, torch.float32, DEV)
    graph.adjacency_cache.entries.clear()
    before = graph.adjacency_cache.flag_reads
    with torch.no_grad():
        for _ in range(2):
            d["edges"] = complete_graph_edges(S, 5, d["loc"].device)
            vc.forward(net, d)
            assert net.last_route == "fused-inference"
    assert graph.adjacency_cache.flag_reads == before + 1
    with torch.no_grad():                                       # the same graph in fresh tensors is a miss: one more read
        d["edges"] = [e.clone() for e in d["edges"]]
        vc.forward(net, d)
    assert graph.adjacency_cache.flag_reads == before + 2
    # a miss while a hipGraph is being captured cannot read the flag back: a clear error, no launch
    d["edges"] = [e.clone() for e in d["edges"]]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"), torch.no_grad():
        vc.forward(net, d)
    assert graph.adjacency_cache.flag_reads == before + 2


def test_adjacency_counts_and_flags():
    from equiadapt_amd import ops

    S = 3
    rows, cols = [e.to(DEV) for e in vc.odd_graph(S)]
    adj, flag = ops.nbody_adjacency(rows, cols, S)
    expect = torch.zeros(5, 5, dtype=torch.int32)
    for r, c in zip([0, 0, 2, 1, 3, 4], [1, 1, 2, 4, 4, 0]):
        expect[c, r] += 1
    assert int(flag.item()) == ops.NBODY_EDGES_OK
    assert torch.equal(adj.cpu(), expect.expand(S, 5, 5))
    bad = {1: (torch.tensor([0, 15, 13]), torch.tensor([1, 2, 14])), 2: (torch.tensor([0, 13]), torch.tensor([5, 14])),
           0: (torch.tensor([0, 1]), torch.tensor([1, 0]))}               # out of range; across systems; last node bare
    for bit, (r, c) in bad.items():
        _, flag = ops.nbody_adjacency(r.to(DEV), c.to(DEV), S)
        got = int(flag.item())
        assert got != ops.NBODY_EDGES_OK and (got & bit) == bit, (bit, got)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_euclidean_group_nbody_on_the_device_matches_the_fp64_cpu_chain():
    S = 6
    hp = dict(vc.DEFAULT, batch_size=S, canon_feature="pv", canon_translation=True)
    torch.manual_seed(14)                                       # frames with cond < 20: see tests/test_vndeepsets.py
    net32 = VNDeepSets(types.SimpleNamespace(**hp), device="cpu").eval()
    g = torch.Generator().manual_seed(13)
    loc, vel = torch.randn(5 * S, 3, generator=g), torch.randn(5 * S, 3, generator=g)
    charges = (torch.randint(0, 2, (5 * S, 1), generator=g) * 2 - 1).float()
    net64 = VNDeepSets(types.SimpleNamespace(**hp), device="cpu").double().eval()
    net64.load_state_dict(net32.state_dict())
    nodes = torch.ones(5 * S, 1)
    with torch.no_grad():
        ref_loc, ref_vel = ea.EuclideanGroupNBody(net64)(nodes.double(), loc=loc.double(), edges=complete_graph_edges(S, 5, "cpu"),
                                                         vel=vel.double(), edge_attr=None, charges=charges.double())
        can = ea.EuclideanGroupNBody(net32.to(DEV))
        out_loc, out_vel = can(nodes.to(DEV), loc=loc.to(DEV), edges=complete_graph_edges(S, 5, DEV), vel=vel.to(DEV), edge_attr=None,
                               charges=charges.to(DEV))
        back = can.invert_canonicalization(out_loc)
    assert net32.last_route == "fused-inference"
    assert (out_loc.double().cpu() - ref_loc).abs().max() <= 5e-5
    assert (out_vel.double().cpu() - ref_vel).abs().max() <= 5e-5
    assert (back.cpu() - loc).abs().max() <= 5e-5
