"""tests/golden/pointcloud_max_train.pt (tests/golden/make_golden_pointcloud_max_train.py: the unmodified reference's
VNSmall(n_knn=20, pooling="max") in train(), dropout p = 0, 4 clouds of 256 points): output, running statistics after the step
and every parameter gradient of sum(out * w).

  * CPU: the package's op-by-op path in fp32 reproduces them, and which parameters get no gradient.  This pins the comparison
    partner of the GPU tests (EQA_TRAIN_FAST=0, the fp64 block of tests/vn_max_cases.py) to the reference.
  * GPU: the fused first block (ConvPosMaxPool) against the same vectors.  Gradients: the yardstick is the op-by-op route on the
    same device, whose per-parameter distance from the reference the fused route may exceed at most twofold (both are fp32
    evaluations and a moved pick hits either), floor 1e-6.
"""
import types

import pytest
import torch


def _net(t, dev):
    import equiadapt_amd as ea

    net = ea.VNSmall(types.SimpleNamespace(n_knn=20, pooling="max"))
    net.load_state_dict(t["state"])
    net.dropout.p = 0.0
    return net.to(dev).train()


def _step(t, dev):
    net = _net(t, dev)
    out = net(t["x"].to(dev))
    (out * t["w"].to(dev)).sum().backward()
    return net, out.detach().cpu()


def _grad_distance(net, t):
    """per parameter: max |grad - reference| relative to the reference's largest entry"""
    d = {}
    for n, p in net.named_parameters():
        if n in t["grads"]:
            g = t["grads"][n]
            d[n] = (p.grad.detach().cpu() - g).abs().max().item() / g.abs().max().item()
    return d


def _check_state_after(net, t, tag):
    after = {k: v.cpu() for k, v in net.state_dict().items()}
    for k, v in t["state_after"].items():
        if v.dtype.is_floating_point:
            assert torch.allclose(after[k], v, atol=1e-6, rtol=1e-5), (tag, k)
        else:
            assert torch.equal(after[k], v), (tag, k)


def test_op_path_on_cpu_reproduces_the_reference(golden):
    t = golden("pointcloud_max_train.pt")
    assert t["provenance"] == "reference" and t["no_grad"] == ["pool.map_to_dir.weight"]
    net, out = _step(t, torch.device("cpu"))
    # the same torch ops in the same order as the reference, fp32 on the same CPU: the bounds of the mean pooling's golden test
    assert torch.allclose(out, t["vnsmall_out"], atol=1e-5, rtol=1e-4)
    _check_state_after(net, t, "cpu")
    assert sorted(n for n, p in net.named_parameters() if p.grad is None) == t["no_grad"]
    for n, e in _grad_distance(net, t).items():
        assert e <= 1e-4, (n, e)


@pytest.mark.gpu
def test_fused_max_training_step_matches_reference_golden(golden, monkeypatch):
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    dev = torch.device("cuda:0")
    t = golden("pointcloud_max_train.pt")
    monkeypatch.delenv("EQA_TRAIN_FAST", raising=False)
    net, out = _step(t, dev)
    err, bound = (out - t["vnsmall_out"]).abs().max().item(), 2e-5 * max(t["vnsmall_out"].abs().max().item(), 1.0)
    print(f"output: {err:.3e} from the reference, bound {bound:.3e}")
    assert err <= bound
    _check_state_after(net, t, "fused")
    assert sorted(n for n, p in net.named_parameters() if p.grad is None) == t["no_grad"]
    fused = _grad_distance(net, t)
    monkeypatch.setenv("EQA_TRAIN_FAST", "0")
    op_net, _ = _step(t, dev)
    monkeypatch.delenv("EQA_TRAIN_FAST")
    op = _grad_distance(op_net, t)
    print("gradient distance from the reference, relative to its largest entry: parameter | op by op | fused")
    for n in fused:
        print(f"  {n} | {op[n]:.3e} | {fused[n]:.3e}")
    for n in fused:
        assert fused[n] <= max(2.0 * op[n], 1e-6), (n, fused[n], op[n])
