"""Bit comparison of two libraries over the four piece forms of the channel contraction, each through its C entry.
  python tools/gemm_bit_compare.py child OUT               -- run the cases with the library EQA_LIB names, write `case digest` lines
  python tools/gemm_bit_compare.py PARENT.so BRANCH.so OUT -- one child per library, compare

Forms: nine and six bf16 piece products (eqa_fft48k5_cgemm3m_bf16x3, block form), the fp16 two-piece form on 32x32x16 and on
16x16x32 matrix instructions (eqa_fft48k5_cgemm3m_f16x2, _k32), at the shapes of tests/test_gpu_cgemm_f16_k32.py.  A digest is the
sha256 of the whole pitched Mo, pre-filled with 7.0, padding included; the split filter pieces are digested too.
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(5, 64, 128), (129, 96, 128), (130, 64, 256), (36, 160, 128)]
MARK = 7.0


def child(out_path):
    import torch

    from equiadapt_amd import _lib
    from equiadapt_amd.images.canonicalization_networks import fftconv

    lib = _lib.load()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    lines = []

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    for (M, Cin, Cout) in SHAPES:
        g = torch.Generator().manual_seed(1000 * M + Cin + Cout)
        bank = (torch.randn(Cout, Cin, 5, 5, generator=g) / (5.0 * Cin ** 0.5)).to(dev)
        B3 = fftconv.filter_spectra3m(bank)
        pitch = lib.eqa_fft48k5_tile_pitch(M)
        V = torch.randn(fftconv.F, pitch, 2 * Cin, generator=g).to(dev)
        slots = torch.zeros(256, device=dev)
        slots[3] = V[:, :M].abs().max()
        slots[77] = slots[3] * 0.25
        bh, b_scale = B3.pieces_f16()
        bk, _ = B3.pieces_f16_k32()
        for name, pieces in (("bf16 pieces", B3.pieces()), ("f16 pieces", bh), ("f16 pieces k32", bk)):
            lines.append(f"{name} {(Cin, Cout)} rc=0 {digest(pieces)}")
        forms = [
            ("9", lambda Mo: lib.eqa_fft48k5_cgemm3m_bf16x3(V.data_ptr(), B3.pieces().data_ptr(), Mo.data_ptr(), M, Cin, Cout, 9, st)),
            ("6", lambda Mo: lib.eqa_fft48k5_cgemm3m_bf16x3(V.data_ptr(), B3.pieces().data_ptr(), Mo.data_ptr(), M, Cin, Cout, 6, st)),
            ("h3/32", lambda Mo: lib.eqa_fft48k5_cgemm3m_f16x2(V.data_ptr(), bh.data_ptr(), Mo.data_ptr(), M, Cin, Cout, slots.data_ptr(), 256, b_scale, st)),
            ("h3/16", lambda Mo: lib.eqa_fft48k5_cgemm3m_f16x2_k32(V.data_ptr(), bk.data_ptr(), Mo.data_ptr(), M, Cin, Cout, slots.data_ptr(), 256, b_scale, st)),
        ]
        for name, run in forms:
            Mo = torch.full((fftconv.F, pitch, 2 * Cout), MARK, device=dev)
            rc = run(Mo)
            lines.append(f"{name} {(M, Cin, Cout)} rc={rc} {digest(Mo) if rc == 0 else '-'}")
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
        results[label] = [l.rsplit(" ", 2) for l in open(path).read().splitlines()]
    a, b = results["parent"], results["branch"]
    assert [x[0] for x in a] == [x[0] for x in b]
    differ = sum(1 for x, y in zip(a, b) if x[1:] != y[1:])
    body = [f"{na} {rca} {da[:16]} {'==' if (rca, da) == (rcb, db) else '!= ' + rcb + ' ' + db[:16]}" for (na, rca, da), (_, rcb, db) in zip(a, b)]
    head = [f"cases: {len(a)} (parent and branch each)", "every digest and status equal" if differ == 0 else f"{differ} CASES DIFFER", "",
            "case status sha256[:16](parent) == / != (branch)"]
    with open(out, "w") as f:
        f.write("\n".join(head + body) + "\n")
    print("\n".join(head[:2]))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        main()
