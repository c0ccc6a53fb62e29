"""fp64 CPU reference of VNSmall's first block with max pooling, shared by tests/test_gpu_vnsmall_max_train.py and
tests/test_vnsmall_max_train_golden.py: conv_pos on the cross edge features of given neighbour lists, then VNMaxPool.

An argmax can move on the last bit of a score, so every comparison against this reference leaves out the entries (cloud, channel,
point) whose two best scores are closer than NEAR_TIE of the largest |score| of the point, and the upstream gradient is zeroed
there (a moved pick then contributes to no gradient sum).  The share left out is capped at MASK_CAP; measured in fp64 with seed 2
weights: 4 x 256 k = 20: 0.31 %, 5 x 200 k = 20: 0.30 %, k = 27: 0.35 %, k = 3: 0.03 %, 3 x 67 k = 7: 0.05 %; no exact ties.
"""
import copy

import torch

NEAR_TIE = 1e-4
MASK_CAP = 0.01
EPS = 1e-6


def fp64_block(conv_pos, pool, x, idx, training, g_up=None):
    """conv_pos: VNLinearLeakyReLU(3 -> 21), pool: VNMaxPool(21) (any device / dtype: copied to the CPU in fp64); x: (B, 3, N);
    idx: (B, N, k) neighbour lists.  Returns a dict: pooled (B, 21, 3, N), pick (B, 21, N) position of the first maximum in the
    list, nbr (B, 21, N) its neighbour id, left_out (B, 21, N) bool near-tie mask, scale / shift (21) of the batch-norm as the
    kernels take them, buffers after the forward, and with g_up (B, 21, 3, N) the parameter gradients of sum(pooled * g_up)
    with g_up zeroed at left_out (grads: name -> tensor or None; g_up: the masked upstream gradient)."""
    from equiadapt_amd.pointcloud.canonicalization_networks.equivariant_networks import get_graph_feature_cross
    from equiadapt_amd.pointcloud.canonicalization_networks.vector_neuron_layers import _mix_channels

    cp = copy.deepcopy(conv_pos).cpu().double().train(training)
    pl = copy.deepcopy(pool).cpu().double()
    for p in list(cp.parameters()) + list(pl.parameters()):
        p.grad = None
    idx = idx.cpu().long()
    B, N, k = idx.shape
    feat = get_graph_feature_cross(x.detach().cpu().double().unsqueeze(1), k, idx)
    bn = cp.batchnorm.bn2d
    with torch.no_grad():
        if training:
            n = torch.norm(_mix_channels(cp.map_to_feat, feat), dim=2) + EPS
            mean, var = n.mean((0, 2, 3)), n.var((0, 2, 3), unbiased=False)
        else:
            mean, var = bn.running_mean.clone(), bn.running_var.clone()
        scale = bn.weight / torch.sqrt(var + bn.eps)
        shift = bn.bias - mean * scale
    h = cp(feat)                                                     # (B, 21, 3, N, k)
    with torch.no_grad():
        s = (h * _mix_channels(pl.map_to_dir, h)).sum(2)             # (B, 21, N, k)
        pick = s.max(dim=-1)[1]                                      # first maximum, as VNMaxPool
        top2 = s.topk(2, dim=-1).values
        left_out = (top2[..., 0] - top2[..., 1]) / s.abs().amax(-1) < NEAR_TIE
    pooled = torch.gather(h, -1, pick[:, :, None, :, None].expand(B, h.shape[1], 3, N, 1)).squeeze(-1)
    out = {"pooled": pooled.detach(), "pick": pick, "nbr": torch.gather(idx[:, None].expand(B, h.shape[1], N, k), -1, pick[..., None]).squeeze(-1),
           "left_out": left_out, "scale": scale, "shift": shift,
           "buffers": {n_: b.detach().clone() for n_, b in cp.named_buffers()}}
    if g_up is not None:
        g = g_up.detach().cpu().double() * (~left_out)[:, :, None, :]
        (pooled * g).sum().backward()
        out["grads"] = {n_: (None if p.grad is None else p.grad.clone()) for n_, p in cp.named_parameters()}
        out["grads"]["pool.map_to_dir.weight"] = pl.map_to_dir.weight.grad
        out["g_up"] = g
    return out
