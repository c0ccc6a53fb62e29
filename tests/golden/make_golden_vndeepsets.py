"""Reference-generated vectors of VNDeepSets, the n-body canonicalization network: tests/golden/vndeepsets.pt (data only).

Run from the repository root (build container only):  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_vndeepsets.py

``equiadapt/nbody/canonicalization_networks/custom_group_equivariant_layers.py`` (VNSoftplus, VNLeakyReLU) is imported UNMODIFIED by
file path: provenance "reference".  ``custom_equivariant_networks.py`` (VNDeepSets) is imported unmodified as well, with a throw-away
``sys.modules["torch_scatter"]`` whose ``scatter`` is the one reduction the file uses, stated in full below: sum or mean over dim 0 by
``index_add_`` into ``index.max() + 1`` rows, the mean dividing by the count clamped to 1.  The label of those cases says so.  The
tests also hold the network to a dense evaluation that uses no scatter at all (tests/test_vndeepsets.py).

Cases, each with S = 6 systems of 5 bodies in eval mode, device "cpu": 1 the yaml default (examples/nbody/configs/canonicalization/
vndeepsets.yaml); 2 pvac / leakyrelu / sum-sum / canon_translation; 3 pv / softplus; 4 prediction mode (out_dim 1); 5 the default on
a ring graph instead of the complete one.  The file is 124 KB: five full state_dicts (2.8 k to 3.0 k parameters each) make up most of it.
"""
import importlib.util
import os
import sys
import types

import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SCATTER_LABEL = "reference source + scatter stand-in (sum / mean by index_add_, length max(index)+1, empty mean 0)"


def scatter(src, index, dim=0, reduce="sum"):
    assert dim == 0 and reduce in ("sum", "mean")
    rows = int(index.max()) + 1
    out = torch.zeros((rows,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
    if reduce == "mean":
        count = torch.zeros(rows, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype)).clamp_(min=1)
        out = out / count.view((rows,) + (1,) * (src.dim() - 1))
    return out


def load_by_path(mod_name: str, rel: str):
    spec = importlib.util.spec_from_file_location(mod_name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[mod_name] = mod
    spec.loader.exec_module(mod)
    return mod


def complete_edges(S):
    r = [i for i in range(5) for j in range(5) if i != j]
    c = [j for i in range(5) for j in range(5) if i != j]
    rows = torch.cat([torch.tensor(r) + 5 * s for s in range(S)])
    cols = torch.cat([torch.tensor(c) + 5 * s for s in range(S)])
    return [rows, cols]


def ring_edges(S):
    rows = torch.cat([torch.arange(5) + 5 * s for s in range(S)])
    cols = torch.cat([(torch.arange(5) + 1) % 5 + 5 * s for s in range(S)])
    return [rows, cols]


DEFAULT = dict(hidden_dim=16, num_layers=4, nonlinearity="relu", canon_feature="p", canon_translation=False, angular_feature=0,
               layer_pooling="mean", final_pooling="mean", out_dim=4, dropout=0.5, batch_size=6)
# Sum pooling multiplies the activations by about four per layer: as initialised, case 2 has outputs up to 200, where one fp32 ulp
# (1.5e-5) is above the 1e-6 the tests hold the plain route to, and two CPUs differ by an ulp or two.  Its parameters and its
# positions / velocities are therefore scaled by 0.25 (stored as scaled: the fixture is the state_dict and the inputs), which puts
# its outputs below 1 like those of the other cases.
SCALE = {"pvac_leakyrelu_sum": 0.25}
CASES = [
    ("default", {}, complete_edges),
    ("pvac_leakyrelu_sum", dict(canon_feature="pvac", nonlinearity="leakyrelu", layer_pooling="sum", final_pooling="sum",
                                canon_translation=True), complete_edges),
    ("pv_softplus", dict(canon_feature="pv", nonlinearity="softplus"), complete_edges),
    ("prediction_mode", dict(out_dim=1), complete_edges),
    ("ring", {}, ring_edges),
]


def main() -> None:
    for pkg in ("equiadapt", "equiadapt.nbody", "equiadapt.nbody.canonicalization_networks"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    layers = load_by_path("equiadapt.nbody.canonicalization_networks.custom_group_equivariant_layers",
                          "equiadapt/nbody/canonicalization_networks/custom_group_equivariant_layers.py")
    ts = types.ModuleType("torch_scatter")
    ts.scatter = scatter
    sys.modules["torch_scatter"] = ts
    nets = load_by_path("equiadapt.nbody.canonicalization_networks.custom_equivariant_networks",
                        "equiadapt/nbody/canonicalization_networks/custom_equivariant_networks.py")

    payload = {"scatter_provenance": SCATTER_LABEL, "cases": {}, "layers": {}}

    # the two nonlinearities on their own: no stand-in involved
    torch.manual_seed(11)
    x = torch.randn(7, 6, 3)
    for name, cls, kw in (("softplus", layers.VNSoftplus, {}), ("leakyrelu", layers.VNLeakyReLU, {}),
                          ("relu", layers.VNLeakyReLU, {"negative_slope": 0.0}),
                          ("leakyrelu_shared", layers.VNLeakyReLU, {"share_nonlinearity": True})):
        mod = cls(6, **kw)
        payload["layers"][name] = {"provenance": "reference", "kwargs": kw, "state": {k: v.clone() for k, v in mod.state_dict().items()},
                                   "x": x, "out": mod(x).detach()}

    for seed, (name, over, edge_fn) in enumerate(CASES):
        hp = dict(DEFAULT, **over)
        torch.manual_seed(100 + seed)
        net = nets.VNDeepSets(types.SimpleNamespace(**hp), device="cpu").eval()
        M = 5 * hp["batch_size"]
        loc, vel, charges = torch.randn(M, 3), torch.randn(M, 3), torch.randint(0, 2, (M, 1)).float() * 2 - 1
        if name in SCALE:
            loc, vel = SCALE[name] * loc, SCALE[name] * vel
            with torch.no_grad():
                for p in net.parameters():
                    p.mul_(SCALE[name])
        edges = edge_fn(hp["batch_size"])
        with torch.no_grad():
            out = net(None, loc, edges, vel, None, charges)
        case = {"provenance": SCATTER_LABEL, "hyperparams": hp, "state": {k: v.clone() for k, v in net.state_dict().items()},
                "loc": loc, "vel": vel, "charges": charges, "edges": edges}
        if hp["out_dim"] == 1:
            case["prediction"] = out.clone()
        else:
            case["rotation_vectors"], case["translation_vectors"] = out[0].clone(), out[1].clone()
        payload["cases"][name] = case

    path = os.path.join(HERE, "vndeepsets.pt")
    torch.save(payload, path)
    print(f"wrote {path}: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
