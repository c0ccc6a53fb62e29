"""Cases, fp64 references and the fp32 CPU yardstick shared by the GPU tests of the fused vector-neuron activation (not a test module).

Reference of every comparison: the plain route in fp64 on the CPU with the same parameters.  Yardstick: the plain route in fp32 on the
CPU; the fused route may be at most 4 x as far from the fp64 result, the fp32 figure taken at run time and pooled over cases.
Errors are the largest absolute difference over max(1, largest absolute fp64 value) of the tensor: inputs and loss weights are N(0, 1),
so outputs and gradients are of order one or larger -- except where the exact result cancels to nearly nothing (C = 1 with a negative
weight and slope 0: y = x EPS / (w^2 |x|^2 + EPS); C = 1 LeakyReLU: dL/dWd is zero where the gate keeps x), and there a figure
relative to the result itself would measure the cancellation in every route, the fp32 yardstick included, or be 0 / 0.

Layouts: (B, C, 3) with B = 1, 5 (P = 1: the point stride is the whole (C, 3) slab); (2, C, 3, N) with N = 63, 64, 65 (one below, on and
one past a wave; with B = 2 a 32-point tile straddles the two batch entries for N = 63, 65) and 257 (past a 256-thread block);
(2, C, 3, 67, 20): P = 1340, 84 tiles with a ragged tail.  C: 1, 5 (below a channel block), 21 (VNSmall's width), 64 (the edge of the
four-channel blocks), 85 (the widest VN-DGCNN layer, eight-channel blocks).  Every C meets every layout; the activation, the shared
direction and the slope rotate so that every C and every layout sees both activations and both kinds of direction map.
"""
import torch

from equiadapt_amd.pointcloud.canonicalization_networks.vector_neuron_layers import VNLeakyReLU, VNSoftplus

FACTOR = 4.0
KINK_COS = 1e-4        # a (b, c, p) whose |cos(x, d)| is below this carries no loss weight in the LeakyReLU gradient tests
MAX_DROPPED = 0.05
CHANNELS = (1, 5, 21, 64, 85)
LAYOUTS = ((1,), (5,), (2, 63), (2, 64), (2, 65), (2, 257), (2, 67, 20))
SLOPES = (0.0, 0.2, 0.1)


def shape_of(C, layout):
    return (layout[0], C, 3) + tuple(layout[1:])


def case(C, layout, softplus, shared, slope, seed):
    name = f"{'softplus' if softplus else 'leaky'}-C{C}-{'shared' if shared else 'own'}-s{slope}-" + "x".join(map(str, shape_of(C, layout)))
    return dict(name=name, C=C, shape=shape_of(C, layout), softplus=softplus, shared=shared, slope=slope, seed=seed)


def _forward_cases():
    cases = []
    for ci, C in enumerate(CHANNELS):
        for li, layout in enumerate(LAYOUTS):
            idx = ci * len(LAYOUTS) + li
            cases.append(case(C, layout, softplus=bool(idx % 2), shared=bool((idx // 2) % 2), slope=SLOPES[idx % 3], seed=idx))
    return cases


FORWARD_CASES = _forward_cases()
for _C in CHANNELS:
    assert {(c["softplus"], c["shared"]) for c in FORWARD_CASES if c["C"] == _C} == {(a, b) for a in (False, True) for b in (False, True)}
for _L in LAYOUTS:
    assert {c["softplus"] for c in FORWARD_CASES if c["shape"][3:] == tuple(_L[1:]) and c["shape"][0] == _L[0]} == {False, True}
assert {c["slope"] for c in FORWARD_CASES} == set(SLOPES)

# every C with both activations and both kinds of direction; the large layout (several tiles per block, ragged tail), a tile that
# straddles two batch entries, and P = 1
BACKWARD_CASES = [
    case(1, (2, 65), False, False, 0.2, 100), case(1, (5,), False, True, 0.0, 101),
    case(5, (2, 67, 20), False, False, 0.0, 102), case(5, (2, 63), False, True, 0.2, 103),
    case(21, (2, 67, 20), False, True, 0.1, 104), case(21, (2, 257), False, False, 0.2, 105),
    case(64, (2, 65), False, False, 0.2, 106), case(64, (2, 67, 20), False, True, 0.0, 107),
    case(85, (2, 67, 20), False, False, 0.2, 108), case(85, (5,), False, True, 0.1, 109),
    case(5, (2, 67, 20), True, False, 0.0, 110), case(5, (1,), True, True, 0.1, 111),
    case(21, (2, 65), True, False, 0.1, 112), case(21, (2, 67, 20), True, True, 0.0, 113),
    case(64, (2, 63), True, True, 0.2, 114), case(85, (2, 67, 20), True, False, 0.0, 115), case(85, (2, 64), True, True, 0.1, 116),
]
SOFTPLUS_C1_CASES = [case(1, (2, 67, 20), True, False, 0.0, 120), case(1, (5,), True, True, 0.1, 121)]


def build(c, dtype, device):
    """The case's module (same parameters for every dtype / device: drawn in fp32 on the CPU), its input and the loss weights r."""
    torch.manual_seed(1000 + c["seed"])
    cls = VNSoftplus if c["softplus"] else VNLeakyReLU
    mod = cls(c["C"], share_nonlinearity=c["shared"], negative_slope=c["slope"])
    g = torch.Generator().manual_seed(2000 + c["seed"])
    x = torch.randn(*c["shape"], generator=g)
    r = torch.randn(*c["shape"], generator=g)
    return mod.to(device=device, dtype=dtype), x.to(device=device, dtype=dtype), r.to(device=device, dtype=dtype)


def rel_error(a, ref):
    """Largest |a - ref| / max(1, max |ref|); over the members of a tuple (VNStdFeature's two outputs) the largest such figure."""
    if isinstance(ref, tuple):
        return max(rel_error(o, r) for o, r in zip(a, ref))
    return float((a.detach().double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def fixture_module(case, dtype=torch.float32):
    """The module of a case of tests/golden/vn_layers_rest.pt with the reference's parameters, in the case's mode."""
    from equiadapt_amd.pointcloud.canonicalization_networks import vector_neuron_layers

    mod = getattr(vector_neuron_layers, case["cls"])(*case["args"], **case["kwargs"])
    mod.load_state_dict(case["state"], strict=True)
    return mod.to(dtype).train(case["train"])


def fixture_yardstick(cases):
    """The reference's own fp32 error against its fp64 output, pooled over the fixture's cases."""
    return max(rel_error(c["out"], c["out64"]) for c in cases.values())


def kink_free(c):
    """(B, C, 1, ...) 0 / 1 in fp64: |cos(x, d)| >= KINK_COS (the LeakyReLU gate's derivative jumps where <x, d> = 0)."""
    mod, x, _ = build(c, torch.float64, "cpu")
    with torch.no_grad():
        d = mod.map_to_dir(x.transpose(1, -1)).transpose(1, -1)
        cos = (x * d).sum(2, keepdim=True) / (x.norm(dim=2, keepdim=True) * d.norm(dim=2, keepdim=True))
    return (cos.abs() >= KINK_COS).double()


def gradients(mod, x, weight):
    """(dL/dx, dL/dWd) for L = sum(y * weight)."""
    mod.map_to_dir.weight.grad = None
    x = x.detach().clone().requires_grad_(True)
    (mod(x) * weight).sum().backward()
    return x.grad.detach(), mod.map_to_dir.weight.grad.detach().clone()
