"""VNSmall(pooling="max") in training on the fused first block (csrc/vnsmall_train.hip: eqa_vn_convpos_max_fwd, _max_bwd_reduce,
_max_bwd_apply; ConvPosMaxPool) against the op-by-op block in fp64 on the CPU (tests/vn_max_cases.py), against the op-by-op
network, and its activation memory.  Near-ties of the argmax are left out of every comparison as vn_max_cases describes; the
share left out must stay below its cap.
"""
import copy
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vn_max_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

NEW_SYMBOLS = ("eqa_vn_convpos_max_fwd", "eqa_vn_convpos_max_bwd_reduce", "eqa_vn_convpos_max_bwd_apply")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    from equiadapt_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _network(dev, k, seed=101):
    import equiadapt_amd as ea

    torch.manual_seed(seed)
    net = ea.VNSmall(types.SimpleNamespace(n_knn=k, pooling="max")).to(dev)
    net.dropout.p = 0.0
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return net


def _apply(net, x, k):
    from equiadapt_amd.pointcloud.canonicalization_networks.equivariant_networks import ConvPosMaxPool

    cp = net.conv_pos
    return ConvPosMaxPool.apply(x, cp.map_to_feat.weight, cp.map_to_dir.weight, cp.batchnorm.bn2d.weight, cp.batchnorm.bn2d.bias,
                                net.pool.map_to_dir.weight, cp.batchnorm.bn2d, k)


def _max_fwd_direct(lib, x, idx, net, scale, shift, k):
    """pooled and sel straight from the entry point, with the batch-norm's scale and shift handed in."""
    B, _, N = x.shape
    cp = net.conv_pos
    pooled = torch.empty(B, 21, 3, N, device=x.device)
    sel = torch.empty(B, 21, N, dtype=torch.uint8, device=x.device)
    sc, sh = scale.float().to(x.device).contiguous(), shift.float().to(x.device).contiguous()
    Wf, Wd, Wp = (w.detach().contiguous() for w in (cp.map_to_feat.weight, cp.map_to_dir.weight, net.pool.map_to_dir.weight))
    assert lib.eqa_vn_convpos_max_fwd(x.data_ptr(), idx.data_ptr(), Wf.data_ptr(), Wd.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                      Wp.data_ptr(), pooled.data_ptr(), sel.data_ptr(), B, N, k, None) == 0
    torch.cuda.synchronize()
    return pooled, sel


def _check_block(dev, B, N, k):
    """ConvPosMaxPool.apply and the forward entry point at one shape, batch-norm in train() and in eval(), against fp64."""
    from equiadapt_amd import _lib
    from equiadapt_amd.pointcloud.canonicalization_networks.equivariant_networks import knn

    lib = _lib.load()
    net = _network(dev, k)
    x = torch.randn(B, 3, N, device=dev)
    g_raw = torch.randn(B, 21, 3, N, device=dev)
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
    assert lib.eqa_vn_knn(x.data_ptr(), idx.data_ptr(), B, N, k, None) == 0
    want = knn(x, k)
    assert torch.equal(idx.long().sort(-1).values, want.sort(-1).values)
    for training in (True, False):
        ref = vc.fp64_block(net.conv_pos, net.pool, x, want, training, g_raw)
        share = ref["left_out"].float().mean().item()
        print(f"B={B} N={N} k={k} train={training}: near-ties left out {100 * share:.3f} %")
        assert share <= vc.MASK_CAP, share
        keep = (~ref["left_out"]).to(dev)
        g_up = ref["g_up"].float().to(dev)
        runs = []
        for _ in range(2):
            fast = copy.deepcopy(net).train(training)
            o = _apply(fast, x, k)
            (o * g_up).sum().backward()
            runs.append((o.detach(), fast))
        (o1, fast), (o1b, fast_b) = runs
        # the same call twice: bit-identical
        assert torch.equal(o1, o1b)
        for p1, p2 in zip(fast.conv_pos.parameters(), fast_b.conv_pos.parameters()):
            assert torch.equal(p1.grad, p2.grad)
        # forward
        err = ((o1.double().cpu() - ref["pooled"]).abs() * (~ref["left_out"])[:, :, None, :]).max().item()
        print(f"  pooled: max error at kept entries {err:.3e}")
        assert err <= 1e-5, (k, training, err)
        # the winner, through the entry point
        pooled_d, sel = _max_fwd_direct(lib, x, idx, net, ref["scale"], ref["shift"], k)
        pooled_d2, sel2 = _max_fwd_direct(lib, x, idx, net, ref["scale"], ref["shift"], k)
        assert torch.equal(sel, sel2) and torch.equal(pooled_d, pooled_d2)
        assert int(sel.max()) < k
        nbr = torch.gather(idx.long()[:, None].expand(B, 21, N, k), -1, sel.long()[..., None]).squeeze(-1)
        moved = ((nbr != ref["nbr"].to(dev)) & keep).sum().item()
        print(f"  picks that differ from fp64 at kept entries: {moved}")
        assert moved == 0, (k, training, moved)
        # backward
        for (name, p1) in fast.conv_pos.named_parameters():
            g2 = ref["grads"][name]
            e = (p1.grad.double().cpu() - g2).abs().max().item() / g2.abs().max().item()
            print(f"  d {name}: {e:.3e} of the largest entry")
            assert e <= 1e-4, (k, training, name, e)
        assert fast.pool.map_to_dir.weight.grad is None and ref["grads"]["pool.map_to_dir.weight"] is None
        for name, b1 in fast.conv_pos.named_buffers():
            assert torch.allclose(b1.double().cpu(), ref["buffers"][name].double(), rtol=1e-5, atol=1e-7), (k, training, name)


@pytest.mark.parametrize("k", [20, 16, 27, 3])
def test_max_block_matches_fp64_block(dev, k):
    """k = 20: every lane busy; 16: idle lanes with E <= 5; 27: the backward's E <= 8 instantiation; 3: fewer edges than lanes."""
    _check_block(dev, 5, 200, k)


@pytest.mark.parametrize("B,N,k", [(3, 67, 7), (1, 20, 20)])
def test_max_block_at_the_edges_of_the_grid(dev, B, N, k):
    """N no multiple of the 32 points of a block; N = k (every point is every point's neighbour)."""
    _check_block(dev, B, N, k)


def test_max_entry_points_check_their_arguments(dev):
    from equiadapt_amd import _lib

    lib = _lib.load()
    N, k = 64, 20
    # B = 0: nothing to do, whatever the pointers
    assert lib.eqa_vn_convpos_max_fwd(None, None, None, None, None, None, None, None, None, 0, N, k, None) == 0
    assert lib.eqa_vn_convpos_max_bwd_reduce(None, None, None, None, None, None, None, None, None, None, None, 0, N, k, None) == 0
    assert lib.eqa_vn_convpos_max_bwd_apply(None, None, None, None, None, None, None, None, None, None, None, None, None, 0, N, k,
                                            None) == 0
    x = torch.randn(1, 3, N, device=dev)
    idx = torch.zeros(1, N, 32, dtype=torch.int32, device=dev)
    w = torch.zeros(21 * 21, device=dev)
    pooled = torch.zeros(1, 21, 3, N, device=dev)
    part = torch.zeros(2 * 21 * 6, device=dev)
    sel = torch.zeros(1, 21, N, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    for kk, s, rc in ((k, None, -1), (33, p(sel), -3)):          # a null sel: invalid argument; k = 33: unsupported
        assert lib.eqa_vn_convpos_max_fwd(p(x), p(idx), p(w), p(w), p(w), p(w), p(w), p(pooled), s, 1, N, kk, None) == rc
        assert lib.eqa_vn_convpos_max_bwd_reduce(p(x), p(idx), p(w), p(w), p(w), p(w), p(w), p(w), p(pooled), s, p(part), 1, N, kk,
                                                 None) == rc
        assert lib.eqa_vn_convpos_max_bwd_apply(p(x), p(idx), p(w), p(w), p(w), p(w), p(w), p(w), p(w), p(w), p(pooled), s, p(part),
                                                1, N, kk, None) == rc
    torch.cuda.synchronize()


def test_max_network_fused_route_matches_op_route(dev, monkeypatch):
    """The whole network, EQA_TRAIN_FAST unset against = 0 (the op-by-op first block), same weights, in train() and in eval()
    with autograd on.  4 x 100 points: more than one block per cloud, N no multiple of 32, and few enough argmax entries
    (8400) that the two fp32 evaluations are not expected to disagree on a pick (2e-5 is the bound without a moved pick)."""
    B, N, k = 4, 100, 20
    net = _network(dev, k, seed=7)
    ref = copy.deepcopy(net)
    x = torch.randn(B, 3, N, device=dev)
    monkeypatch.delenv("EQA_TRAIN_FAST", raising=False)
    for training in (True, False):
        net.train(training)
        ref.train(training)
        w = torch.randn(B, 3, 3, device=dev)
        for p in list(net.parameters()) + list(ref.parameters()):
            p.grad = None
        a1 = net(x)
        monkeypatch.setenv("EQA_TRAIN_FAST", "0")
        a2 = ref(x)
        monkeypatch.delenv("EQA_TRAIN_FAST")
        err = (a1 - a2).abs().max().item()
        print(f"train={training}: output differs by {err:.3e}, bound {2e-5 * max(a2.abs().max().item(), 1.0):.3e}")
        assert err <= 2e-5 * max(a2.abs().max().item(), 1.0)
        (a1 * w).sum().backward()
        (a2 * w).sum().backward()
        for (n1, p1), (n2, p2) in zip(net.named_parameters(), ref.named_parameters()):
            assert (p1.grad is None) == (p2.grad is None), n1
            if p2.grad is None:
                continue
            g = max(p2.grad.abs().max().item(), 1e-6)
            e = (p1.grad - p2.grad).abs().max().item()
            print(f"  d {n1}: {e / g:.3e} of the largest entry")
            assert e <= 5e-2 * g, (training, n1, e, g)
        assert net.pool.map_to_dir.weight.grad is None
        for (n1, b1), (n2, b2) in zip(net.named_buffers(), ref.named_buffers()):
            assert torch.allclose(b1.float(), b2.float(), rtol=1e-4, atol=1e-6), n1


def test_new_symbols_are_exported(dev):
    from equiadapt_amd import _lib

    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_max_training_step_keeps_no_edge_tensor(dev, monkeypatch):
    """B = 8, N = 1024, k = 20, train(), forward + backward: the step's peak allocation stays below ONE (B, 21, 3, N, k) fp32
    tensor (41.3 MB).  The fused route allocates idx, pooled, sel, the tail's g_pooled and mask and per-block partials (< 10 MB);
    the op-by-op first block keeps several tensors of that size for autograd."""
    monkeypatch.delenv("EQA_TRAIN_FAST", raising=False)
    B, N, k = 8, 1024, 20
    net = _network(dev, k).train()
    x = torch.randn(B, 3, N, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = net(x)
    out.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    one_edge_tensor = B * 21 * 3 * N * k * 4
    print(f"peak allocation of the step: {peak / 1e6:.2f} MB (one edge tensor: {one_edge_tensor / 1e6:.1f} MB)")
    assert peak < one_edge_tensor, (peak, one_edge_tensor)
