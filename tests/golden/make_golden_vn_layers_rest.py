"""Reference-generated vectors of the vector-neuron layers VNSmall does not use: tests/golden/vn_layers_rest.pt (data only).

Run from the repository root (build container only), with the reference checkout's root as the argument:
    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_golden_vn_layers_rest.py <reference root>

``equiadapt/pointcloud/canonicalization_networks/vector_neuron_layers.py`` is imported UNMODIFIED by file path (it needs torch only):
provenance "reference".  Every case stores the input, the state_dict, the reference's fp32 output ("out") and the output of the same
module after ``.double()`` on the fp64 input ("out64"): the yardstick and the reference of the tests (VNBilinear casts its labels to
fp32, so its "out64" is nn.functional.bilinear in fp64 on the reference module's weight).  VNStdFeature returns
(x_std, z0); both are stored.  Every batch size is 2 or 4: for B = 3 the reference's ``torch.cross`` without ``dim`` takes the batch axis.

Cases: VNLinear(5, 7) on 4-D, 5-D and 3-D inputs; VNLeakyReLU and VNSoftplus with and without share_nonlinearity; VNBilinear(6, 4, 7);
VNStdFeature(8, dim) for dim 3, 4, 5 with and without normalize_frame in eval mode (batch-norm buffers and affine parameters
randomised as in make_golden.py), and one dim = 4 case in train mode with the state_dict after the step.
"""
import copy
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def load_reference(root: str):
    path = os.path.join(root, "equiadapt/pointcloud/canonicalization_networks/vector_neuron_layers.py")
    spec = importlib.util.spec_from_file_location("reference_vector_neuron_layers", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def randomise_batchnorm(module) -> None:
    for mod in module.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.running_mean.normal_(0.5, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.2)


def detach(out):
    return tuple(o.detach().clone() for o in out) if isinstance(out, tuple) else out.detach().clone()


def record(mod, inputs, train: bool = False):
    """fp32 output of the module as it stands, fp64 output of a .double() copy from the same state."""
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    mod64 = copy.deepcopy(mod).double()
    mod.train(train)
    mod64.train(train)
    with torch.no_grad():
        out = detach(mod(*inputs))
        if type(mod).__name__ == "VNBilinear":
            # the reference's forward casts the labels to fp32, so the .double() module cannot run: its one op in fp64 on its weights
            x64, labels64 = (t.double() for t in inputs)
            out64 = torch.nn.functional.bilinear(x64.transpose(1, -1), labels64.repeat(1, x64.shape[2], 1),
                                                 mod64.map_to_feat.weight).transpose(1, -1).clone()
        else:
            out64 = detach(mod64(*[t.double() for t in inputs]))
    case = {"provenance": "reference", "inputs": [t.clone() for t in inputs], "state": state, "train": train, "out": out, "out64": out64}
    if train:
        case["state_after"] = {k: v.clone() for k, v in mod.state_dict().items()}
        case["state_after64"] = {k: v.clone() for k, v in mod64.state_dict().items() if "running" in k}
    return case


def main(root: str) -> None:
    vnl = load_reference(root)
    cases = {}
    specs = [
        ("linear_4d", "VNLinear", (5, 7), {}, [(2, 5, 3, 9)]),
        ("linear_5d", "VNLinear", (5, 7), {}, [(2, 5, 3, 9, 4)]),
        ("linear_3d", "VNLinear", (5, 7), {}, [(4, 5, 3)]),
        ("leakyrelu_4d", "VNLeakyReLU", (5,), {"negative_slope": 0.2}, [(2, 5, 3, 9)]),
        ("leakyrelu_shared_5d", "VNLeakyReLU", (5,), {"share_nonlinearity": True, "negative_slope": 0.0}, [(2, 5, 3, 9, 4)]),
        ("leakyrelu_shared_3d", "VNLeakyReLU", (5,), {"share_nonlinearity": True, "negative_slope": 0.0}, [(4, 5, 3)]),
        ("softplus_4d", "VNSoftplus", (5,), {}, [(2, 5, 3, 9)]),
        ("softplus_shared_5d", "VNSoftplus", (5, True, 0.1), {}, [(2, 5, 3, 9, 4)]),
        ("bilinear_3d", "VNBilinear", (6, 4, 7), {}, [(2, 6, 3), (2, 1, 4)]),
    ]
    for seed, (name, cls, args, kw, shapes) in enumerate(specs):
        torch.manual_seed(300 + seed)
        mod = getattr(vnl, cls)(*args, **kw)
        case = record(mod, [torch.randn(*s) for s in shapes])
        case.update({"cls": cls, "args": args, "kwargs": kw})
        cases[name] = case
    std_shapes = {3: (4, 8, 3), 4: (2, 8, 3, 6), 5: (2, 8, 3, 5, 3)}
    seed = 400
    for dim in (3, 4, 5):
        for frame in (False, True):
            torch.manual_seed(seed)
            seed += 1
            mod = vnl.VNStdFeature(8, dim=dim, normalize_frame=frame)
            randomise_batchnorm(mod)
            case = record(mod, [torch.randn(*std_shapes[dim])])
            case.update({"cls": "VNStdFeature", "args": (8,), "kwargs": {"dim": dim, "normalize_frame": frame}})
            cases[f"stdfeature_dim{dim}_{'frame' if frame else 'free'}"] = case
    torch.manual_seed(seed)
    mod = vnl.VNStdFeature(8, dim=4, normalize_frame=True)
    randomise_batchnorm(mod)
    case = record(mod, [torch.randn(4, 8, 3, 6)], train=True)
    case.update({"cls": "VNStdFeature", "args": (8,), "kwargs": {"dim": 4, "normalize_frame": True}})
    cases["stdfeature_dim4_train"] = case

    path = os.path.join(HERE, "vn_layers_rest.pt")
    torch.save({"provenance": "reference", "cases": cases}, path)
    print(f"wrote {path}: {os.path.getsize(path)} B")


if __name__ == "__main__":
    main(sys.argv[1])
