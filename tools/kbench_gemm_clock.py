"""The shader clock the piece contractions (block form) sustain, and how their cycles divide: both kernels of the fp16 form "h3"
(v_mfma_f32_32x32x16_f16 with K-stages of 16, v_mfma_f32_16x16x32_f16 with K-stages of 32) alternated in one process, three runs
each, and the bf16 forms (9 / 6 products) once.

A variant build of the library (-DEQA_BLK_CLOCK=1: first / last s_memtime and the constant 100 MHz counter of one wave; =2: an
s_memtime at region boundaries of a K-stage as well) exports eqa_debug_blk_clock.  The product library has none of this: on it
the tool prints the times alone.

    python -c "from equiadapt_amd import _lib; _lib.build(extra_flags=['-DEQA_BLK_CLOCK=1'], out='build_variants/libeqa_clock.so')"
    EQA_LIB=build_variants/libeqa_clock.so python tools/kbench_gemm_clock.py

Operands: the headline shape (1024 tiles, 256 -> 256 channels), V and Mo taken in turn from a ring of buffers of 2.4 GB each, so no
launch finds its operands in a cache.  Every timing follows `--warm` launches of the same kernel (the clock settles under load).
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from equiadapt_amd import _lib                                                     # noqa: E402
from equiadapt_amd.images.canonicalization_networks import fftconv as fc          # noqa: E402

STAMPED_BLOCK = 100          # BlkClock::publish (csrc/cgemm3m_pieces.inc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ring", type=int, default=2)
    args = ap.parse_args()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.SO_PATH)
    stamped = hasattr(raw, "eqa_debug_blk_clock")
    out = (ctypes.c_longlong * 10)()
    dev = torch.device("cuda:0")
    M, Cin, Cout = 1024, 256, 256
    # the block tiles of the stamped block: XCD b % 8 holds the frequencies f % 8 == b % 8, its 32 blocks deal their tiles round robin
    xcd, q = STAMPED_BLOCK % 8, STAMPED_BLOCK // 8
    tiles = len(range(q, -(-(fc.F - xcd) // 8) * (-(-M // 128)) * (Cout // 128), 32))
    g = torch.Generator().manual_seed(0)
    bank = (torch.randn(Cout, Cin, 5, 5, generator=g) / (5.0 * Cin ** 0.5)).to(dev)
    B = fc.filter_spectra3m(bank)
    Mos = [fc.spectra_buffer(M, 2 * Cout, dev) for _ in range(args.ring)]
    st = torch.cuda.current_stream().cuda_stream
    print(f"library {_lib.SO_PATH}; {fc.F} x [{M} x {Cin}].[{Cin} x {Cout}]; block {STAMPED_BLOCK}: {tiles} tiles; "
          f"{args.warm} launches, then {args.reps} timed, ring of {args.ring}")
    # kernel: (label, K of a stage, matrix instructions per stage and wave, cycles of one)
    kernels = {"h3/32x32x16": (16, 36, 32), "h3/16x16x32": (32, 144, 16), "9": (16, 108, 32), "6": (16, 72, 32)}
    for what in ("random operands", "A = 0"):
        Vs = [fc.spectra_buffer(M, 2 * Cin, dev) for _ in range(args.ring)]
        for V in Vs:
            V.normal_() if what == "random operands" else V.zero_()
        vb = torch.ones(1, device=dev) * 8.0
        turn = [0]

        def run(kernel):
            V, Mo = Vs[turn[0] % args.ring], Mos[turn[0] % args.ring]
            turn[0] += 1
            if kernel == "h3/32x32x16":
                bh, b_scale = B.pieces_f16()
                _lib.check(lib.eqa_fft48k5_cgemm3m_f16x2(V.data_ptr(), bh.data_ptr(), Mo.data_ptr(), M, Cin, Cout, vb.data_ptr(), 1, b_scale, st), "f16x2")
            elif kernel == "h3/16x16x32":
                bk, b_scale = B.pieces_f16_k32()
                _lib.check(lib.eqa_fft48k5_cgemm3m_f16x2_k32(V.data_ptr(), bk.data_ptr(), Mo.data_ptr(), M, Cin, Cout, vb.data_ptr(), 1, b_scale, st),
                           "f16x2_k32")
            else:
                _lib.check(lib.eqa_fft48k5_cgemm3m_bf16x3(V.data_ptr(), B.pieces().data_ptr(), Mo.data_ptr(), M, Cin, Cout, int(kernel), st), "bf16x3")

        order = ["h3/32x32x16", "h3/16x16x32"] * args.runs + (["9", "6"] if what == "random operands" else [])
        for kernel in order:
            k_stage, n_mfma, c_mfma = kernels[kernel]
            for _ in range(args.warm):
                run(kernel)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                run(kernel)
            b.record()
            torch.cuda.synchronize()
            line = f"{what:>16}, {kernel:>12}: {a.elapsed_time(b) / args.reps:6.3f} ms per launch"
            if stamped:
                raw.eqa_debug_blk_clock(out)
                stages = tiles * (Cin // k_stage)
                line += (f"; mfma {n_mfma} per stage of {k_stage} k; block {STAMPED_BLOCK}: {out[0]} cycles = {out[0] / stages * (32 // k_stage):6.0f} per 32 k "
                         f"(matrix instructions {n_mfma * c_mfma * (32 // k_stage)}: {n_mfma * c_mfma * stages / out[0]:.2f} of the cycles), "
                         f"{out[0] / (out[1] * 10.0):5.3f} GHz, tile epilogue {out[2] / tiles:5.0f} cycles")
                if out[3]:
                    line += f", regions per stage {[round(out[3 + i] / stages) for i in range(5)]}"
            print(line, flush=True)


if __name__ == "__main__":
    main()
