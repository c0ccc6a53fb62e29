"""Reference-generated training-mode vectors of VNSmall with pooling="max": output, running statistics after the step and the
gradient of every parameter (pool.map_to_dir.weight has none: it only feeds the argmax).

Run from the repository root (build container only):  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_pointcloud_max_train.py

Same procedure and provenance as tests/golden/make_golden_pointcloud1024.py: the reference's
``equiadapt/pointcloud/canonicalization_networks/{vector_neuron_layers,equivariant_networks}.py`` and ``equiadapt/common/*.py``
are imported UNMODIFIED by file path; ``omegaconf`` (absent here, used by those files only as a type annotation) is a throw-away
module object whose ``DictConfig`` is never called.  The fixture holds data only: inputs, parameters, expected outputs.

Case (seeded): VNSmall(n_knn=20, pooling="max"), seed 2, dropout p = 0, train(); x = randn(4, 3, 256), seed 0; w = randn(4, 3, 3).
"""
import importlib.util
import os
import sys
import types

import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def load_by_path(mod_name: str, rel: str):
    spec = importlib.util.spec_from_file_location(mod_name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[mod_name] = mod
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    for pkg in ("equiadapt", "equiadapt.common", "equiadapt.pointcloud", "equiadapt.pointcloud.canonicalization_networks"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    load_by_path("equiadapt.common.utils", "equiadapt/common/utils.py")
    load_by_path("equiadapt.pointcloud.canonicalization_networks.vector_neuron_layers",
                 "equiadapt/pointcloud/canonicalization_networks/vector_neuron_layers.py")
    oc = types.ModuleType("omegaconf")

    class DictConfig:  # never instantiated or called by the code under test
        pass

    oc.DictConfig = DictConfig
    sys.modules["omegaconf"] = oc
    eqn = load_by_path("equiadapt.pointcloud.canonicalization_networks.equivariant_networks",
                       "equiadapt/pointcloud/canonicalization_networks/equivariant_networks.py")

    torch.manual_seed(2)
    net = eqn.VNSmall(types.SimpleNamespace(n_knn=20, pooling="max"))
    net.dropout.p = 0.0            # deterministic; the dropout mask is torch's own RNG stream either way
    net.train()
    torch.manual_seed(0)
    x = torch.randn(4, 3, 256)
    w = torch.randn(4, 3, 3)
    st0 = {n: v.clone() for n, v in net.state_dict().items()}
    out = net(x)
    (out * w).sum().backward()
    payload = {"provenance": "reference", "B": 4, "N": 256, "k": 20, "pooling": "max",
               "state": st0, "x": x, "w": w, "vnsmall_out": out.detach(),
               "state_after": {n: v.clone() for n, v in net.state_dict().items()},
               "grads": {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None},
               "no_grad": sorted(n for n, p in net.named_parameters() if p.grad is None)}
    path = os.path.join(HERE, "pointcloud_max_train.pt")
    torch.save(payload, path)
    print(f"wrote {path}: {os.path.getsize(path)} B; no gradient: {payload['no_grad']}")


if __name__ == "__main__":
    main()
