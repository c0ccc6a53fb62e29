"""Bit comparison of two libraries over every branch of the FFT launch plan.
  python tools/fft_bit_compare.py child OUT      -- run the cases with the library EQA_LIB names, write `case digest` lines
  python tools/fft_bit_compare.py PARENT.so BRANCH.so OUT  -- children for both libraries under three environments, compare
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENVS = [("default", {}), ("inv_pipe_0", {"EQA_FFT_INV_PIPE": "0"}), ("two_pass", {"EQA_FFT_TWO_PASS": "1"})]
MARK = 7.0


def child(out_path):
    import torch

    from equiadapt_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda")
    F = lib.eqa_fft48k5_frequencies()
    lines = []
    gen = torch.Generator(device=dev)

    def rnd(n, seed):
        gen.manual_seed(seed)
        return torch.randn(int(n), device=dev, generator=gen)

    def marked(n, dtype=torch.float32):
        return torch.full((max(int(n), 1),), MARK, dtype=dtype, device=dev)

    def digest(*ts):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in ts:
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()

    def rec(name, rc, *outs):
        lines.append(f"{name} rc={rc} {digest(*outs) if rc == 0 else '-'}")

    def tiles(n, k):
        return lib.eqa_fft48_tiles(n, k)

    def ws(nimg, rows, cols, C, k):
        return marked(max(lib.eqa_fft48_workspace_bytes(nimg, rows, cols, C, k), 4) // 4)

    def spec(M, width):
        return (lib.eqa_fft48k5_tile_pitch(M) if M > 0 else 1) * F * width

    def call(fam, name, k, *args):
        """fam 'k5': eqa_fft48k5_<name>(*args, stream); 'any': eqa_fft48_<name>(*args, k, stream)"""
        if fam == "k5":
            return getattr(lib, "eqa_fft48k5_" + name)(*args, None)
        return getattr(lib, "eqa_fft48_" + name)(*args, k, None)

    def forward_cases(fam, k, nimg, C, H, W, tag=""):
        OH, OW = H - k + 1, W - k + 1
        M = nimg * tiles(H, k) * tiles(W, k)
        x = rnd(nimg * H * W * C, 1)
        ib = rnd(C, 2)
        for act in (0, 1):
            names = ["input"] + (["input_grouped"] if fam == "k5" else [])
            for name in names:
                T, V = ws(nimg, H, OW, C, k), marked(spec(M, 2 * C))
                rc = call(fam, name, k, x.data_ptr(), T.data_ptr(), V.data_ptr(), ib.data_ptr() if act else None, act, nimg, H, W, C)
                rec(f"{fam} {name}{tag} k={k} n={nimg} C={C} {H}x{W} act={act}", rc, V)
        # gradient tiles: the map is the OUTPUT gradient
        Mg = nimg * tiles(H + k - 1, k) * tiles(W + k - 1, k)
        T, G = ws(nimg, H, W, C, k), marked(spec(Mg, 2 * C))
        rc = call(fam, "grad_transform", k, x.data_ptr(), T.data_ptr(), G.data_ptr(), nimg, H, W, C)
        rec(f"{fam} grad_transform{tag} k={k} n={nimg} C={C} {H}x{W}", rc, G)

    def output_cases(fam, k, nimg, C, OH, OW):
        H, W = OH + k - 1, OW + k - 1
        TY, TX = tiles(H, k), tiles(W, k)
        M = nimg * TY * TX
        Mo = rnd(spec(M, 2 * C), 3)
        bias = rnd(C, 4)
        for act in (0, 1):
            T2, y = ws(nimg, OH, OW, C, k), marked(nimg * OH * OW * C)
            rc = call(fam, "output", k, Mo.data_ptr(), T2.data_ptr(), bias.data_ptr() if act else None, act, y.data_ptr(), nimg, OH, OW, C)
            rec(f"{fam} output k={k} n={nimg} C={C} {OH}x{OW} act={act}", rc, y)
        if fam != "k5":
            return
        rows = lib.eqa_fft48k5_output_stats_rows(nimg, OH, OW, C)
        T2, y, part = ws(nimg, OH, OW, C, k), marked(nimg * OH * OW * C), marked(max(rows, 1) * C * 2, torch.float64)
        rc = lib.eqa_fft48k5_output_stats(Mo.data_ptr(), T2.data_ptr(), y.data_ptr(), part.data_ptr(), nimg, OH, OW, C, None)
        rec(f"k5 output_stats n={nimg} C={C} {OH}x{OW} rows={rows}", rc, y, part)
        for kn in (3, 5):
            for act in (0, 1):
                T2, S = ws(nimg, OH, OW, C, k), marked(nimg * C * kn * kn, torch.float64)
                wsp = marked(nimg * OH * TX * C * (2 * kn - 1))
                rc = lib.eqa_fft48k5_output_sums(Mo.data_ptr(), T2.data_ptr(), bias.data_ptr() if act else None, act, S.data_ptr(), wsp.data_ptr(),
                                                 nimg, OH, OW, C, kn, None)
                rec(f"k5 output_sums n={nimg} C={C} {OH}x{OW} k_next={kn} act={act}", rc, S)

    def input_grad_cases(fam, k, nimg, C, H, W):
        TY, TX = tiles(H, k), tiles(W, k)
        M = nimg * TY * TX
        Cg = rnd(spec(M, 2 * C), 5)
        T2, dx = ws(nimg, 48 * TY, W - k + 1, C, k), marked(nimg * H * W * C)
        rc = call(fam, "input_grad", k, Cg.data_ptr(), T2.data_ptr(), dx.data_ptr(), nimg, H, W, C)
        rec(f"{fam} input_grad k={k} n={nimg} C={C} {H}x{W}", rc, dx)

    def filter_cases(fam, k, Cin, Cout):
        bank = rnd(Cout * Cin * k * k, 6)
        D = rnd(F * 2 * Cin * 2 * Cout, 7)
        for corr in (0, 1):
            B = marked(F * 2 * Cin * 2 * Cout)
            rc = (lib.eqa_fft48k5_filter_spectra(bank.data_ptr(), B.data_ptr(), Cout, Cin, corr, None) if fam == "k5" else
                  lib.eqa_fft48_filter_spectra(bank.data_ptr(), B.data_ptr(), Cout, Cin, k, corr, None))
            rec(f"{fam} filter_spectra k={k} Cin={Cin} Cout={Cout} correlate={corr}", rc, B)
            B3 = marked(max(lib.eqa_fft48k5_spectra3m_floats(Cin, Cout), 4))
            rc = (lib.eqa_fft48k5_filter_spectra3m(bank.data_ptr(), B3.data_ptr(), Cout, Cin, corr, None) if fam == "k5" else
                  lib.eqa_fft48_filter_spectra3m(bank.data_ptr(), B3.data_ptr(), Cout, Cin, k, corr, None))
            rec(f"{fam} filter_spectra3m k={k} Cin={Cin} Cout={Cout} correlate={corr}", rc, B3)
        for packed in (0, 1):
            db = marked(Cout * Cin * k * k)
            if fam == "k5":
                fn = lib.eqa_fft48k5_filter_grad3m if packed else lib.eqa_fft48k5_filter_grad
                rc = fn(D.data_ptr(), db.data_ptr(), Cout, Cin, None)
            else:
                rc = lib.eqa_fft48_filter_grad(D.data_ptr(), db.data_ptr(), Cout, Cin, k, packed, None)
            rec(f"{fam} filter_grad k={k} Cin={Cin} Cout={Cout} packed={packed}", rc, db)

    maps = [(92, 92), (53, 50), (20, 33), (137, 49)]
    for C in (8, 16, 48):
        for (H, W) in maps:
            forward_cases("k5", 5, 2, C, H, W)
            input_grad_cases("k5", 5, 2, C, H, W)
        for (H, W) in maps + [(15, 50), (11, 50)]:
            output_cases("k5", 5, 2, C, H - 4, W - 4)
    output_cases("k5", 5, 25, 48, 88, 88)              # 100 tiles x 3 channel groups: the pipeline's blocks take one or two items
    os.environ["EQA_FFT_FWD_PIPE"] = "1"               # read per call: 128 x 4 tiles x 4 groups = 2048 work items
    forward_cases("k5", 5, 128, 64, 92, 92, tag="[FWD_PIPE=1]")
    forward_cases("k5", 5, 2, 16, 92, 92, tag="[FWD_PIPE=1]")
    del os.environ["EQA_FFT_FWD_PIPE"]
    for (Cin, Cout) in [(8, 12), (64, 64), (512, 16)]:
        filter_cases("k5", 5, Cin, Cout)
        for k in (3, 5, 7, 9):
            filter_cases("any", k, Cin, Cout)
    for k in (3, 5, 7, 9):
        for C in (16, 24):
            for (H, W) in [(56, 56), (60, 97)]:
                forward_cases("any", k, 2, C, H, W)
                input_grad_cases("any", k, 2, C, H, W)
                output_cases("any", k, 2, C, H - k + 1, W - k + 1)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} cases written to {out_path}")


def main():
    parent, branch, out = sys.argv[1:4]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    results = {}
    for label, so in (("parent", parent), ("branch", branch)):
        for env_name, extra in ENVS:
            path = f"{out}.{label}.{env_name}"
            env = dict(os.environ, EQA_LIB=os.path.abspath(so), **extra)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=env, timeout=500)
            if res.returncode != 0:
                sys.exit(f"child {label} {env_name} ended with {res.returncode}: nothing more is started")
            results[(label, env_name)] = [l.rsplit(" ", 2) for l in open(path).read().splitlines()]
    total = differ = 0
    body = []
    for env_name, extra in ENVS:
        a, b = results[("parent", env_name)], results[("branch", env_name)]
        body.append(f"\n## environment: {env_name} {extra if extra else ''}")
        assert len(a) == len(b)
        for (na, rca, da), (nb, rcb, db) in zip(a, b):
            assert na == nb
            total += 1
            same = rca == rcb and da == db
            differ += 0 if same else 1
            body.append(f"{na} {rca} {da[:16]} {'==' if same else '!= ' + rcb + ' ' + db[:16]}")
    head = [f"cases: {total} (parent and branch each, three environments)", "every digest and status equal" if differ == 0 else f"{differ} CASES DIFFER",
            "", "case status sha256[:16](parent) == / != (branch); rc=-3: the entry point declines the shape (EQA_ERR_UNSUPPORTED), in both libraries"]
    with open(out, "w") as f:
        f.write("\n".join(head + body) + "\n")
    print("\n".join(head[:2]))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        main()
