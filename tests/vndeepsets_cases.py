"""Cases, fp64 references and the fp32 CPU yardstick shared by the VNDeepSets GPU tests (not a test module).

Reference of every comparison: the plain route in fp64 on the CPU with the same parameters.  Yardstick: the same route in fp32 on
the CPU; the fused route may be at most 4 x as far from the fp64 result, the fp32 figure taken at run time and pooled over cases.
"""
import types

import torch

from equiadapt_amd.nbody import complete_graph_edges
from equiadapt_amd.nbody.canonicalization_networks import VNDeepSets

DEFAULT = dict(hidden_dim=16, num_layers=4, nonlinearity="relu", canon_feature="p", canon_translation=False, angular_feature=0,
               layer_pooling="mean", final_pooling="mean", out_dim=4, dropout=0.5)
KINK_COS = 1e-4           # a system with an activation whose |cos(z, d)| is below this carries no loss weight in the gradient tests
MAX_DROPPED = 0.05


def odd_graph(S):
    """Per system: 0->1 twice, a self-loop on 2, 1->4, 3->4, 4->0; body 3 has no incoming edge."""
    src, dst = [0, 0, 2, 1, 3, 4], [1, 1, 2, 4, 4, 0]
    return [torch.cat([torch.tensor(src) + 5 * s for s in range(S)]), torch.cat([torch.tensor(dst) + 5 * s for s in range(S)])]


def ring_graph(S):
    return [torch.cat([torch.arange(5) + 5 * s for s in range(S)]), torch.cat([(torch.arange(5) + 1) % 5 + 5 * s for s in range(S)])]


def edges_of(graph, S):
    if graph == "k5":
        return [e.clone() for e in complete_graph_edges(S, 5, "cpu")]
    return {"ring": ring_graph, "odd": odd_graph}[graph](S)


def case(name, S, graph="k5", seed=0, train=False, **over):
    return dict(name=name, S=S, graph=graph, seed=seed, train=train, hp=dict(DEFAULT, batch_size=S, **over))


# S: 1 (one system in a wave), 4 (a full wave), 5 (one past it), 67 (several blocks, ragged tail).  H: 16 and 32 (compiled widths), 5
# (odd; L = 1), 12 and 20, which run zero-padded to the widths 8, 16 and 32.  L: 1, 4, 8.
FORWARD_CASES = [
    case("default-S1", 1),
    case("pv-leaky-ring-S4", 4, "ring", canon_feature="pv", nonlinearity="leakyrelu"),
    case("pvac-sum-odd-S5", 5, "odd", canon_feature="pvac", layer_pooling="sum", final_pooling="sum", canon_translation=True),
    case("default-S67", 67),
    case("H5-L1-pvac-odd-S67", 67, "odd", hidden_dim=5, num_layers=1, canon_feature="pvac", nonlinearity="leakyrelu",
         final_pooling="sum", canon_translation=True),
    case("H32-L8-pv-S5", 5, hidden_dim=32, num_layers=8, canon_feature="pv"),
    case("H32-L1-sum-ring-S67", 67, "ring", hidden_dim=32, num_layers=1, nonlinearity="leakyrelu", layer_pooling="sum"),
    case("L8-pva-odd-S4", 4, "odd", num_layers=8, canon_feature="pva"),
    case("softplus-pv-S5", 5, canon_feature="pv", nonlinearity="softplus"),
    case("softplus-H32-pvac-ring-S67", 67, "ring", hidden_dim=32, canon_feature="pvac", nonlinearity="softplus", canon_translation=True),
    case("softplus-H5-L1-odd-S1", 1, "odd", hidden_dim=5, num_layers=1, nonlinearity="softplus", layer_pooling="sum",
         final_pooling="sum"),
    case("H12-L2-pvc-S4", 4, hidden_dim=12, num_layers=2, canon_feature="pvc"),
    case("H20-L3-leaky-odd-S5", 5, "odd", hidden_dim=20, num_layers=3, nonlinearity="leakyrelu", canon_translation=True),
]

# S = 1030: 258 groups of four systems on the backward's 256 blocks, so two blocks add a second group to their partial sums.
BACKWARD_CASES = [
    case("default-S67-eval", 67),
    case("default-S67-train", 67, train=True),
    case("H32-L8-pv-leaky-ring-S5-train", 5, "ring", train=True, hidden_dim=32, num_layers=8, canon_feature="pv", nonlinearity="leakyrelu"),
    case("H5-L1-pvac-leaky-sum-odd-S4-eval", 4, "odd", hidden_dim=5, num_layers=1, canon_feature="pvac", nonlinearity="leakyrelu",
         layer_pooling="sum", final_pooling="sum", canon_translation=True),
    case("pvac-odd-S1-train", 1, "odd", train=True, canon_feature="pvac", final_pooling="sum", canon_translation=True),
    case("H12-L2-pvc-leaky-ring-S67-eval", 67, "ring", hidden_dim=12, num_layers=2, canon_feature="pvc", nonlinearity="leakyrelu",
         layer_pooling="sum"),
    case("H20-L3-pva-S5-train", 5, train=True, hidden_dim=20, num_layers=3, canon_feature="pva"),
    case("default-S1030-eval", 1030),
    case("default-S4096-train", 4096, train=True),        # the benchmark's larger size: every backward block adds four groups
]


def build(c, dtype, device):
    """The case's network (same parameters for every dtype / device: drawn in fp32 on the CPU), inputs and edges."""
    torch.manual_seed(1000 + c["seed"])
    net = VNDeepSets(types.SimpleNamespace(**c["hp"]), device="cpu")
    g = torch.Generator().manual_seed(2000 + c["seed"])
    M = 5 * c["S"]
    loc, vel = torch.randn(M, 3, generator=g), torch.randn(M, 3, generator=g)
    charges = (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1).float()
    hp = c["hp"]
    mask = None
    if c["train"]:
        keep = 1.0 - hp["dropout"]
        mask = (torch.rand(hp["num_layers"], M, 3, hp["hidden_dim"], generator=g) < keep).float() / keep
    wr, wt = torch.randn(M, 3, 3, generator=g), torch.randn(M, 3, generator=g)
    net = net.to(device=device, dtype=dtype)
    net.train(c["train"])
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)      # noqa: E731
    edges = [e.to(device) for e in edges_of(c["graph"], c["S"])]
    return net, dict(loc=to(loc), vel=to(vel), charges=to(charges), edges=edges, mask=to(mask), wr=to(wr), wt=to(wt))


def forward(net, d):
    return net(None, d["loc"], d["edges"], d["vel"], None, d["charges"], _dropout_mask=d["mask"])


def kink_free_systems(c):
    """(S,) bool in fp64: no activation of the system has |cos(z, d)| below KINK_COS (the gradient jumps where <z, d> = 0)."""
    net, d = build(c, torch.float64, "cpu")
    worst = []

    def hook(mod, args):
        x = args[0]                                                     # (M, H, 3)
        dirs = mod.map_to_dir(x.transpose(1, -1)).transpose(1, -1)
        cos = (x * dirs).sum(2) / (x.norm(dim=2) * dirs.norm(dim=2))
        worst.append(cos.abs().min(dim=1).values)

    handles = [m.nonlinear_function.register_forward_pre_hook(hook) for m in net._layers()]
    with torch.no_grad():
        forward(net, d)
    for h in handles:
        h.remove()
    per_node = torch.stack(worst).min(dim=0).values
    return per_node.view(c["S"], 5).min(dim=1).values >= KINK_COS


def gradients(net, d, system_weight):
    """Gradient of every parameter tensor for the fixed linear functional sum(wr * rot) + sum(wt * trans), systems weighted."""
    for p in net.parameters():
        p.grad = None
    rot, trans = forward(net, d)
    w = system_weight.to(rot).repeat_interleave(5)
    loss = (rot * d["wr"] * w[:, None, None]).sum() + (trans * d["wt"] * w[:, None]).sum()
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}
