"""Bit comparison of two libraries over the point-cloud VN kernels (eval forward, canonicalizer, a VNSmall training step).
  python tools/vn_bit_compare.py child OUT               -- run the cases with the library EQA_LIB names, write `case digest` lines
  python tools/vn_bit_compare.py PARENT.so BRANCH.so OUT -- a fresh child process per library, compare
"""
import hashlib
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (k, B, N): N = k (one block, all padding) | ragged, two quad blocks, N no multiple of 16 | two single-kernel blocks of 128 |
# a lane with a short share | the SEG = 8 instantiation (twice) | small k
FWD_SHAPES = [(20, 1, 20), (20, 2, 70), (20, 2, 130), (19, 2, 64), (21, 2, 100), (32, 2, 32), (3, 2, 70)]


def child(out_path):
    import torch

    import equiadapt_amd as ea
    from equiadapt_amd import _lib, ops

    lib = _lib.load()
    dev = torch.device("cuda")
    lines = []

    def digest(*ts):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in ts:
            h.update(t.detach().cpu().numpy().tobytes())
        return h.hexdigest()

    def net_and_cloud(k, pooling, B, N):
        torch.manual_seed(1000 * k + N)
        net = ea.VNSmall(types.SimpleNamespace(n_knn=k, pooling=pooling)).to(dev)
        with torch.no_grad():   # running statistics and affine terms away from their initial 0 / 1
            for m in net.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    m.running_mean.uniform_(0.2, 0.6)
                    m.running_var.uniform_(0.5, 1.5)
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.3, 0.3)
        return net, torch.randn(B, 3, N, device=dev)

    for pooling in ("mean", "max"):
        for (k, B, N) in FWD_SHAPES:
            net, x = net_and_cloud(k, pooling, B, N)
            prm = net.eval().packed_parameters()
            for choice in ((0, 1, 2) if k == 20 else (0,)):   # eqa_set_option key 1: default, one thread per point, four lanes
                lib.eqa_set_option(1, choice)
                try:
                    lines.append(f"vnsmall_fwd {pooling} k={k} B={B} N={N} choice={choice} {digest(ops.vnsmall_forward(x, prm, k, pooling))}")
                finally:
                    lib.eqa_set_option(1, 0)
        for N in (64, 70):   # float4 tail | scalar tail
            net, x = net_and_cloud(20, pooling, 2, N)
            vec, R, y = ops.vnsmall_canonicalize(x, net.eval().packed_parameters(), 20, pooling)
            lines.append(f"vnsmall_canonicalize {pooling} k=20 B=2 N={N} {digest(vec, R, y)}")
        for k in (20, 27):
            net, x = net_and_cloud(k, pooling, 2, 70)
            net.train()
            torch.manual_seed(7)   # the dropout mask
            out = net(x)
            (out * torch.linspace(-1.0, 1.0, out.numel(), device=dev).view_as(out)).sum().backward()
            # every parameter in name order; one without a gradient (W_p of VNMaxPool only feeds the argmax) counts as zeros
            grads = [p.grad if p.grad is not None else torch.zeros_like(p) for _, p in sorted(net.named_parameters())]
            assert sum(float(g.abs().sum()) > 0 for g in grads) >= 12, "the step reached too few parameters"
            lines.append(f"vnsmall_train_step {pooling} k={k} B=2 N=70 {digest(out, *grads)}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} cases written to {out_path}")


def main():
    parent, branch, out = sys.argv[1:4]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    results = {}
    for label, so in (("parent", parent), ("branch", branch)):
        path = f"{out}.{label}"
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=dict(os.environ, EQA_LIB=os.path.abspath(so)),
                             timeout=300)
        if res.returncode != 0:
            sys.exit(f"child {label} ended with {res.returncode}: nothing more is started")
        results[label] = [l.rsplit(" ", 1) for l in open(path).read().splitlines()]
    a, b = results["parent"], results["branch"]
    assert [n for n, _ in a] == [n for n, _ in b]
    differ = sum(1 for (_, da), (_, db) in zip(a, b) if da != db)
    head = [f"cases: {len(a)} (parent and branch each)", "every digest equal" if differ == 0 else f"{differ} CASES DIFFER", "",
            "case sha256[:16](parent) == / != (branch)"]
    body = [f"{na} {da[:16]} {'==' if da == db else '!= ' + db[:16]}" for (na, da), (_, db) in zip(a, b)]
    with open(out, "w") as f:
        f.write("\n".join(head + body) + "\n")
    print("\n".join(head[:2]))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        main()
