"""Inputs, the loss and the CPU chains shared by the n-body frame tests and the golden generator (not a test module).

Frames: rows of randn(3,3) from a seeded CPU generator, a row redrawn while its condition number exceeds MAX_COND, so nothing is
excluded afterwards.  Reference of every comparison: autograd through EuclideanGroupNBody's own op-by-op path in fp64 on the CPU;
yardstick: the same path in fp32 on the CPU (tests/test_gpu_nbody_frame.py).
"""
import torch

MAX_COND = 20.0
SIZES = (1, 5, 255, 256, 257, 1030)      # one thread, one system, the three sides of a block edge, several blocks + a ragged tail
GOLDEN_SIZES = (15, 257)
INPUT_NAMES = ("v", "t", "loc", "vel")


def frames(M, generator):
    v = torch.randn(M, 3, 3, generator=generator)
    while True:
        bad = torch.linalg.cond(v) > MAX_COND
        n = int(bad.sum())
        if n == 0:
            return v
        v[bad] = torch.randn(n, 3, 3, generator=generator)


def inputs(M, seed=0):
    """fp32 CPU tensors: the frame vectors v, t, loc, vel and the fixed weights w1, w2, w3 (M,3), wR (M,3,3)."""
    g = torch.Generator().manual_seed(7000 + 13 * M + seed)
    d = {"v": frames(M, g)}
    for name in ("t", "loc", "vel", "w1", "w2", "w3"):
        d[name] = torch.randn(M, 3, generator=g)
    d["wR"] = torch.randn(M, 3, 3, generator=g)
    return d


class TwoParameters(torch.nn.Module):
    """Stand-in network: returns its two parameters (rotation vectors, translation vectors)."""

    def __init__(self, v, t):
        super().__init__()
        self.v, self.t = torch.nn.Parameter(v.clone()), torch.nn.Parameter(t.clone())

    def forward(self, nodes, loc, edges, vel, edge_attr, charges):
        return self.v, self.t


class SlicedParameter(torch.nn.Module):
    """Stand-in network: one (M,3,4) parameter, returned as two strided views like VNDeepSets' plain route."""

    def __init__(self, v, t):
        super().__init__()
        self.out = torch.nn.Parameter(torch.cat([v, t[:, :, None]], dim=2))

    def forward(self, nodes, loc, edges, vel, edge_attr, charges):
        return self.out[:, :, :3], self.out[:, :, 3]


def run(can, loc, vel):
    nodes = torch.ones(loc.shape[0], 1, dtype=loc.dtype, device=loc.device)
    return can(nodes, loc=loc, edges=None, vel=vel, edge_attr=None, charges=None)


def golden_loss(can, cloc, cvel, w1, w2, w3, node_weight=None):
    """sum(w1 cloc) + sum(w2 cvel) + sum(w3 invert(0.5 cloc + cvel)); returns (loss, inverted)."""
    M = w1.shape[0]
    inverted = can.invert_canonicalization(0.5 * cloc.reshape(M, 3) + cvel.reshape(M, 3)).reshape(M, 3)
    k = 1.0 if node_weight is None else node_weight[:, None]
    return (k * w1 * cloc.reshape(M, 3)).sum() + (k * w2 * cvel.reshape(M, 3)).sum() + (k * w3 * inverted).sum(), inverted


def golden_chain(cls, d, dtype, device="cpu", network=TwoParameters):
    """The class ``cls`` (this package's or the reference's) with a stand-in network on the inputs ``d``: outputs and the gradients
    of the golden loss with respect to v, t, loc, vel (for SlicedParameter: "out" instead of v and t)."""
    to = lambda x: x.detach().to(device=device, dtype=dtype).clone()      # noqa: E731
    net = network(to(d["v"]), to(d["t"])).to(device)
    can = cls(net)
    loc, vel = to(d["loc"]).requires_grad_(True), to(d["vel"]).requires_grad_(True)
    cloc, cvel = run(can, loc, vel)
    R = can.canonicalization_info_dict["group_element"]["rotation_matrix"]
    loss, inverted = golden_loss(can, cloc, cvel, to(d["w1"]), to(d["w2"]), to(d["w3"]))
    loss.backward()
    M = loc.shape[0]
    out = {"R": R.detach(), "cloc": cloc.detach().reshape(M, 3), "cvel": cvel.detach().reshape(M, 3), "inverted": inverted.detach()}
    grads = {name: p.grad.detach().clone() for name, p in net.named_parameters()}
    grads["loc"], grads["vel"] = loc.grad.detach().clone(), vel.grad.detach().clone()
    return can, out, grads


def frame_chain(cls, d, dtype, use=("wR", "w1", "w2"), need_rows=True):
    """Op-by-op on the CPU: gradients of sum(wR R) + sum(w1 cloc) + sum(w2 cvel), restricted to the weights in ``use``, with respect
    to v, t (and loc, vel if ``need_rows``)."""
    to = lambda x: x.detach().to(dtype=dtype).clone()      # noqa: E731
    net = TwoParameters(to(d["v"]), to(d["t"]))
    can = cls(net)
    loc, vel = to(d["loc"]).requires_grad_(need_rows), to(d["vel"]).requires_grad_(need_rows)
    cloc, cvel = run(can, loc, vel)
    M = loc.shape[0]
    R = can.canonicalization_info_dict["group_element"]["rotation_matrix"]
    terms = {"wR": R, "w1": cloc.reshape(M, 3), "w2": cvel.reshape(M, 3)}
    sum((to(d[k]) * terms[k]).sum() for k in use).backward()
    grads = {"v": net.v.grad, "t": net.t.grad}
    if need_rows:
        grads["loc"], grads["vel"] = loc.grad, vel.grad
    return {k: (torch.zeros_like(to(d[k])) if g is None else g.detach().clone()) for k, g in grads.items()}


def invert_chain(d, R, dtype):
    """Op-by-op x R + t on the CPU with x = loc: gradients of sum(w3 out) with respect to x and R."""
    x, R = d["loc"].to(dtype).clone().requires_grad_(True), R.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = torch.bmm(x[:, None, :], R).reshape(-1, 3) + d["t"].to(dtype)
    (d["w3"].to(dtype) * out).sum().backward()
    return {"x": x.grad, "R": R.grad}


def rel_error(got, ref64):
    """max |got - ref| relative to the tensor's largest fp64 entry."""
    return float((got.double().cpu() - ref64).abs().max() / ref64.abs().max())
