"""Reference-generated outputs and gradients of the n-body canonicalizer's frame chain: tests/golden/nbody_frame_grads.pt (data only).

Run from the repository root (build container only):  PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_nbody_frame.py

``equiadapt/common/utils.py``, ``equiadapt/common/basecanonicalization.py`` and ``equiadapt/nbody/canonicalization/euclidean_group.py``
are torch-only and are imported UNMODIFIED by file path, at generation time only: provenance "reference".  The canonicalization
network is a stand-in that returns two parameters (tests/nbody_frame_cases.py TwoParameters), so the gradients with respect to the
rotation vectors v and the translation vectors t are those parameters' gradients.

Per M in (15, 257), in fp32 and in fp64 (the fp64 inputs are the fp32 ones widened): v, t, loc, vel and the weights w1, w2, w3; the
outputs R, cloc, cvel of ``canonicalize`` and inverted = ``invert_canonicalization(0.5 cloc + cvel)``; the gradients of
sum(w1 cloc) + sum(w2 cvel) + sum(w3 inverted) with respect to v, t, loc, vel.  Frames: tests/nbody_frame_cases.py (cond <= 20).
"""
import importlib.util
import os
import sys
import types

import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))                       # tests/: nbody_frame_cases

import nbody_frame_cases as fc  # noqa: E402


def load_by_path(mod_name: str, rel: str):
    spec = importlib.util.spec_from_file_location(mod_name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[mod_name] = mod
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    for pkg in ("equiadapt", "equiadapt.common", "equiadapt.nbody", "equiadapt.nbody.canonicalization"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    load_by_path("equiadapt.common.utils", "equiadapt/common/utils.py")
    load_by_path("equiadapt.common.basecanonicalization", "equiadapt/common/basecanonicalization.py")
    nb = load_by_path("equiadapt.nbody.canonicalization.euclidean_group", "equiadapt/nbody/canonicalization/euclidean_group.py")

    payload = {"provenance": "reference", "max_cond": fc.MAX_COND, "cases": {}}
    for M in fc.GOLDEN_SIZES:
        d = fc.inputs(M)
        case = {}
        for label, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
            _, out, grads = fc.golden_chain(nb.EuclideanGroupNBody, d, dtype)
            case[label] = {"inputs": {k: d[k].to(dtype) for k in ("v", "t", "loc", "vel", "w1", "w2", "w3")},
                           "outputs": out, "grads": {k: grads[k] for k in fc.INPUT_NAMES}}
        payload["cases"][M] = case
    path = os.path.join(HERE, "nbody_frame_grads.pt")
    torch.save(payload, path)
    print(f"wrote {path}: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
