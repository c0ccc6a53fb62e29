"""CPU-only: VNDeepSets (the n-body canonicalization network) on its plain route -- against reference-generated vectors, against a
dense evaluation that uses neither scatter nor package code, and against the symmetries it has (and the one it lacks)."""
import types

import pytest
import torch

import equiadapt_amd as ea
from equiadapt_amd.nbody import complete_graph_edges
from equiadapt_amd.nbody.canonicalization_networks import SequentialMultiple, VNDeepSetLayer, VNDeepSets, VNLeakyReLU, VNSoftplus
from equiadapt_amd.nbody.canonicalization_networks import custom_group_equivariant_layers as vn_layers

DEFAULT = dict(hidden_dim=16, num_layers=4, nonlinearity="relu", canon_feature="p", canon_translation=False, angular_feature=0,
               layer_pooling="mean", final_pooling="mean", out_dim=4, dropout=0.5, batch_size=6)


def hyper(**over):
    return types.SimpleNamespace(**dict(DEFAULT, **over))


def odd_graph(S):
    """Per system: 0->1 twice, a self-loop on 2, 1->4, 3->4, 4->0; body 3 has no incoming edge (and is not the last node)."""
    src, dst = [0, 0, 2, 1, 3, 4], [1, 1, 2, 4, 4, 0]
    rows = torch.cat([torch.tensor(src) + 5 * s for s in range(S)])
    cols = torch.cat([torch.tensor(dst) + 5 * s for s in range(S)])
    return [rows, cols]


def ring_graph(S):
    rows = torch.cat([torch.arange(5) + 5 * s for s in range(S)])
    cols = torch.cat([(torch.arange(5) + 1) % 5 + 5 * s for s in range(S)])
    return [rows, cols]


def inputs(S, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    M = 5 * S
    return (torch.randn(M, 3, generator=g, dtype=dtype), torch.randn(M, 3, generator=g, dtype=dtype),
            (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1).to(dtype))


def make_net(seed=0, dtype=torch.float64, **over):
    torch.manual_seed(seed)
    return VNDeepSets(hyper(**over), device="cpu").to(dtype).eval()


def run(net, loc, vel, charges, edges):
    with torch.no_grad():
        return net(None, loc, edges, vel, None, charges)


# ------------------------------------------------------------------------------------------------------------ golden vectors
def test_layers_reproduce_the_reference(golden):
    g = golden("vndeepsets.pt")
    assert vn_layers.EPS == 1e-6
    for name, case in g["layers"].items():
        assert case["provenance"] == "reference"
        cls = VNSoftplus if name == "softplus" else VNLeakyReLU
        mod = cls(6, **case["kwargs"])
        mod.load_state_dict(case["state"], strict=True)
        assert torch.allclose(mod(case["x"]), case["out"], rtol=0, atol=1e-6), name
    assert VNSoftplus(4).negative_slope == 0.0 and VNLeakyReLU(4).negative_slope == 0.2
    assert VNLeakyReLU(4, share_nonlinearity=True).map_to_dir.weight.shape == (1, 4)


@pytest.mark.parametrize("name", ["default", "pvac_leakyrelu_sum", "pv_softplus", "prediction_mode", "ring"])
def test_plain_route_reproduces_the_reference_cases(golden, name):
    case = golden("vndeepsets.pt")["cases"][name]
    assert "scatter stand-in" in case["provenance"]
    net = VNDeepSets(types.SimpleNamespace(**case["hyperparams"]), device="cpu").eval()
    assert list(net.state_dict().keys()) == list(case["state"].keys())
    assert all(net.state_dict()[k].shape == v.shape for k, v in case["state"].items())
    net.load_state_dict(case["state"], strict=True)
    out = run(net, case["loc"], case["vel"], case["charges"], case["edges"])
    assert net.last_route.startswith("plain")
    if name == "prediction_mode":
        assert out.shape == case["prediction"].shape == (30, 3)
        assert (out - case["prediction"]).abs().max() <= 1e-6
    else:
        assert out[0].shape == (30, 3, 3) and out[1].shape == (30, 3)
        assert (out[0] - case["rotation_vectors"]).abs().max() <= 1e-6
        assert (out[1] - case["translation_vectors"]).abs().max() <= 1e-6


def test_attributes_and_state_dict_keys():
    net = VNDeepSets(dict(DEFAULT, learning_rate=1e-3), device="cpu")        # a dict is accepted as the image classes accept one
    assert net.model == "vndeepsets" and net.prediction_mode is False and net.in_dim == 1
    assert net.learning_rate == 1e-3 and net.weight_decay == 0.0 and net.patience == 100
    assert isinstance(net.set_layers, SequentialMultiple) and isinstance(net.first_set_layer, VNDeepSetLayer)
    keys = list(net.state_dict().keys())
    assert keys[:5] == ["first_set_layer.identity_linear.weight", "first_set_layer.identity_linear.bias",
                        "first_set_layer.pooling_linear.weight", "first_set_layer.pooling_linear.bias",
                        "first_set_layer.nonlinear_function.map_to_dir.weight"]
    assert "set_layers.2.nonlinear_function.map_to_dir.weight" in keys and keys[-2:] == ["output_layer.weight", "output_layer.bias"]
    assert len(keys) == 5 * 4 + 2                                            # dummy_input / dummy_indices are plain attributes
    assert net.dummy_input.dtype == torch.long and net.dummy_indices.shape == (1,)
    assert ea.VNDeepSets is VNDeepSets and "VNDeepSets" in ea.__all__ and ea.nbody.VNDeepSets is VNDeepSets
    assert VNDeepSets(hyper(canon_feature="pvac"), device="cpu").in_dim == 4


def test_complete_graph_edges():
    rows, cols = complete_graph_edges(2, 5, "cpu")
    assert rows[:20].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4]
    assert cols[:20].tolist() == [1, 2, 3, 4, 0, 2, 3, 4, 0, 1, 3, 4, 0, 1, 2, 4, 0, 1, 2, 3]
    assert torch.equal(rows[20:], rows[:20] + 5) and torch.equal(cols[20:], cols[:20] + 5)
    again = complete_graph_edges(2, 5, "cpu")
    assert again[0] is rows and again[1] is cols


# -------------------------------------------------------------------------------------------------------- dense definition
def dense_eval(net, hp, loc, vel, charges, edges):
    """The network from its state_dict alone: 5 x 5 adjacency matrices per system and loops over bodies; no scatter, no package code."""
    sd = {k: v.double() for k, v in net.state_dict().items()}
    S, H, L = hp.batch_size, hp.hidden_dim, hp.num_layers
    slope = {"relu": 0.0, "leakyrelu": 0.2}.get(hp.nonlinearity)
    A = torch.zeros(S, 5, 5, dtype=torch.float64)            # A[s, target, source]
    for r, c in zip(edges[0].tolist(), edges[1].tolist()):
        assert r // 5 == c // 5
        A[r // 5, c % 5, r % 5] += 1
    rot, trans = torch.zeros(5 * S, 3, 3, dtype=torch.float64), torch.zeros(5 * S, 3, dtype=torch.float64)
    for s in range(S):
        P, V, Q = loc[5 * s:5 * s + 5].double(), vel[5 * s:5 * s + 5].double(), charges[5 * s:5 * s + 5].double()
        centre = P.sum(0) / (5 if hp.layer_pooling == "mean" else 1)
        feats = []
        for b in range(5):
            p = P[b] - centre
            ang = torch.stack([p[1] * V[b][2] - p[2] * V[b][1], p[2] * V[b][0] - p[0] * V[b][2], p[0] * V[b][1] - p[1] * V[b][0]])
            table = {"p": p, "v": V[b], "a": ang, "c": p * Q[b]}
            feats.append(torch.stack([table[ch] for ch in hp.canon_feature], dim=1))          # (3, Cin)
        x = feats
        for l in range(L):
            pre = "first_set_layer." if l == 0 else f"set_layers.{l - 1}."
            WI, bI = sd[pre + "identity_linear.weight"], sd[pre + "identity_linear.bias"]
            WP, bP = sd[pre + "pooling_linear.weight"], sd[pre + "pooling_linear.bias"]
            Wd = sd[pre + "nonlinear_function.map_to_dir.weight"]
            new = []
            for b in range(5):
                pooled = torch.zeros_like(x[b])
                for j in range(5):
                    pooled = pooled + A[s, b, j] * x[j]
                if hp.layer_pooling == "mean":
                    pooled = pooled / max(float(A[s, b].sum()), 1.0)
                z = x[b] @ WI.T + bI + pooled @ WP.T + bP          # (3, H): the bias lands on every spatial component
                d = z @ Wd.T
                out = torch.zeros_like(z)
                for ch in range(H):
                    zc, dc = z[:, ch], d[:, ch]
                    dot, dd = (zc * dc).sum(), (dc * dc).sum()
                    proj = zc - dot / (dd + 1e-6) * dc
                    if slope is None:
                        mask = torch.cos(torch.acos(dot / (zc.norm() * dc.norm() + 1e-6)) / 2) ** 2
                        out[:, ch] = mask * zc + (1 - mask) * proj
                    else:
                        out[:, ch] = slope * zc + (1 - slope) * (zc if dot >= 0 else proj)
                new.append(out + x[b] if l > 0 else out)
            x = new
        pooled = sum(x) / (5 if hp.final_pooling == "mean" else 1)
        o = pooled @ sd["output_layer.weight"].T + sd["output_layer.bias"]         # (3, 4)
        for b in range(5):
            rot[5 * s + b] = o[:, :3]
            trans[5 * s + b] = (o[:, 3] if hp.canon_translation else 0.0) + centre
    return rot, trans


@pytest.mark.parametrize("over, graph", [
    ({}, "complete"), ({}, "odd"), (dict(layer_pooling="sum", final_pooling="sum", canon_feature="pvac", nonlinearity="leakyrelu",
                                         canon_translation=True), "odd"),
    (dict(canon_feature="pv", nonlinearity="softplus", hidden_dim=5, num_layers=2), "ring"),
    (dict(canon_feature="pvc", layer_pooling="sum", hidden_dim=7, num_layers=3), "ring"),
    (dict(canon_feature="pva", final_pooling="sum", num_layers=1), "odd"),
])
def test_plain_route_equals_a_dense_evaluation_in_fp64(over, graph):
    S = 4
    hp = hyper(batch_size=S, **over)
    net = make_net(seed=3, **dict(over, batch_size=S))
    loc, vel, charges = inputs(S, seed=5)
    edges = {"complete": complete_graph_edges(S, 5, "cpu"), "odd": odd_graph(S), "ring": ring_graph(S)}[graph]
    rot, trans = run(net, loc, vel, charges, edges)
    ref_rot, ref_trans = dense_eval(net, hp, loc, vel, charges, edges)
    assert rot.dtype == torch.float64
    assert (rot - ref_rot).abs().max() <= 1e-12
    assert (trans - ref_trans).abs().max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------- properties
def test_translation_equivariance():
    S = 3
    net = make_net(seed=1, batch_size=S, canon_feature="pvac", canon_translation=True)
    loc, vel, charges = inputs(S, seed=2)
    edges = complete_graph_edges(S, 5, "cpu")
    shift = torch.tensor([0.7, -1.3, 2.1], dtype=torch.float64)
    rot, trans = run(net, loc, vel, charges, edges)
    rot2, trans2 = run(net, loc + shift, vel, charges, edges)
    assert (rot2 - rot).abs().max() <= 1e-12
    assert (trans2 - (trans + shift)).abs().max() <= 1e-12


def _rotation(seed):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    return q * torch.sign(torch.linalg.det(q))


def test_rotation_equivariance_holds_only_with_zero_biases():
    S = 3
    net = make_net(seed=4, batch_size=S, canon_feature="pva")
    loc, vel, charges = inputs(S, seed=6)
    edges = complete_graph_edges(S, 5, "cpu")
    R = _rotation(7)

    def defect():
        rot, _ = run(net, loc, vel, charges, edges)
        rot2, _ = run(net, loc @ R.T, vel @ R.T, charges, edges)
        return float((rot2 - torch.einsum("ij,mjk->mik", R, rot)).abs().max())

    as_initialised = defect()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.zero_()
    assert defect() <= 1e-12
    assert as_initialised > 1e-3, "the biases of the reference's nn.Linear layers break rotation equivariance: the docstring says so"


def test_permuting_the_bodies_of_a_system_changes_nothing():
    S = 3
    net = make_net(seed=8, batch_size=S, canon_feature="pvac", canon_translation=True)
    loc, vel, charges = inputs(S, seed=9)
    edges = odd_graph(S)
    perm = torch.tensor([3, 0, 4, 1, 2])                            # body b moves to slot perm[b]
    node_map = torch.cat([perm + 5 * s for s in range(S)])
    loc2, vel2, ch2 = torch.empty_like(loc), torch.empty_like(vel), torch.empty_like(charges)
    loc2[node_map], vel2[node_map], ch2[node_map] = loc, vel, charges
    edges2 = [node_map[edges[0]], node_map[edges[1]]]
    # (the last node of the permuted graph must keep an incoming edge: old body 2 lands there, and it has its self-loop)
    rot, trans = run(net, loc, vel, charges, edges)
    rot2, trans2 = run(net, loc2, vel2, ch2, edges2)
    assert (rot2[::5] - rot[::5]).abs().max() <= 1e-12
    assert (trans2[::5] - trans[::5]).abs().max() <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- errors
def test_wrong_node_count_is_a_value_error():
    net = make_net(batch_size=4)
    loc, vel, charges = inputs(3, seed=0)
    with pytest.raises(ValueError, match="5 bodies"):
        net(None, loc, complete_graph_edges(3, 5, "cpu"), vel, None, charges)


def test_last_node_without_incoming_edge_is_the_shape_error_of_the_reference():
    S = 2
    net = make_net(batch_size=S)
    loc, vel, charges = inputs(S, seed=0)
    rows, cols = complete_graph_edges(S, 5, "cpu")
    keep = cols != 5 * S - 1
    with pytest.raises(RuntimeError, match="size of tensor"):
        run(net, loc, vel, charges, [rows[keep], cols[keep]])


# ------------------------------------------------------------------------------------------------------------ end to end
def test_euclidean_group_nbody_with_vndeepsets_on_cpu():
    S = 6
    torch.manual_seed(14)
    net = VNDeepSets(hyper(batch_size=S, canon_feature="pv", canon_translation=True), device="cpu").eval()
    can = ea.EuclideanGroupNBody(net)
    loc, vel, charges = inputs(S, seed=13, dtype=torch.float32)
    # The round trip is (loc - t) R^T R + t with R the fp32 Gram-Schmidt frame of the three predicted vectors V: its defect from
    # orthonormality is about cond(V) * 2^-24 per unit of |loc| (|loc| up to 3 here).  An untrained network predicts frames with
    # cond(V) from 10 to 10^4 depending on the seed; 1e-5 needs cond(V) below about 50.  The seed is chosen for that, and the
    # condition is asserted so that a change of initialisation shows up here and not as a round-trip failure.
    with torch.no_grad():
        vectors, _ = net(None, loc, complete_graph_edges(S, 5, "cpu"), vel, None, charges)
    assert float(torch.linalg.cond(vectors[::5].double()).max()) < 20
    with torch.no_grad():
        canonical_loc, canonical_vel = can(torch.ones(5 * S, 1), loc=loc, edges=complete_graph_edges(S, 5, "cpu"), vel=vel, edge_attr=None,
                                           charges=charges)
        back = can.invert_canonicalization(canonical_loc)
    assert canonical_loc.shape == loc.shape and canonical_vel.shape == vel.shape
    R = can.canonicalization_info_dict["group_element"]["rotation_matrix"]
    assert (R @ R.transpose(1, 2) - torch.eye(3)).abs().max() <= 1e-5
    assert (back - loc).abs().max() <= 1e-5
