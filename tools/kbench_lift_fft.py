"""The fused lifting convolution + forward FFT-48 transform (eqa_lift5_fft48k5_input, csrc/lift_fft.hip) against the two kernels it
replaces (eqa_lift_conv_grouped then eqa_fft48k5_input_grouped) at the headline shape, back to back, per launch.

    python tools/kbench_lift_fft.py [--batch 256] [--channels 256]
With a library built with -DEQA_LF_CLOCK (EQA_LIB=...): also the per-phase shader cycles of block 0.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from equiadapt_amd import _lib, ops                                                   # noqa: E402
from equiadapt_amd.images.canonicalization_networks import fftconv as fc             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--h2-only", action="store_true", help="time the default (two fp16 pieces) form alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, C, S = a.batch, a.channels, a.size
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, S, S, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    bank = (torch.randn(C, 3, 5, 5, generator=g) / 75 ** 0.5).to(dev).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(C, generator=g).to(dev)
    wpk = ops.pack_lift_weights(bank)
    H1 = S - 4
    M = B * fc.tiles(H1) ** 2
    st = torch.cuda.current_stream().cuda_stream
    V = fc.spectra_buffer(M, 2 * C, dev)
    T = torch.empty(max(lib.eqa_fft48k5_workspace_bytes(B, H1, H1 - 4, C), 4) // 4, dtype=torch.float32, device=dev)

    def fused():
        _lib.check(lib.eqa_lift5_fft48k5_input(x.data_ptr(), bank.data_ptr(), bias.data_ptr(), 1, V.data_ptr(), B, S, S, C, st), "fused")

    from equiadapt_amd.images.canonicalization_networks.fftconv import LiftedInput
    wp = LiftedInput(x, bank, bias, True).pieces()

    def fused_p():
        _lib.check(lib.eqa_lift5_fft48k5_input_bf16x3(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), 1, V.data_ptr(), B, S, S, C, st), "fused bf16x3")

    wh, w_scale = LiftedInput(x, bank, bias, True).pieces_f16()
    xb = torch.empty(256, dtype=torch.float32, device=dev)
    dcm = torch.empty(256, dtype=torch.float32, device=dev)

    def fused_h():
        _lib.check(lib.eqa_absmax_slots(x.data_ptr(), x.numel(), xb.data_ptr(), st), "absmax")
        _lib.check(lib.eqa_lift5_fft48k5_input_f16x2(x.data_ptr(), wh.data_ptr(), w_scale, xb.data_ptr(), 256, bias.data_ptr(), 1, V.data_ptr(),
                                                     dcm.data_ptr(), B, S, S, C, st), "fused f16x2")

    def two():
        y = ops.lift_conv_grouped(x, wpk, bias, True, 5, 5)
        _lib.check(lib.eqa_fft48k5_input_grouped(y.data_ptr(), T.data_ptr(), V.data_ptr(), None, 0, B, H1, H1, C, st), "grouped")

    def lift_only():
        ops.lift_conv_grouped(x, wpk, bias, True, 5, 5)

    forms = (("fused eqa_lift5_fft48k5_input", fused), ("fused eqa_lift5_fft48k5_input_bf16x3", fused_p),
             ("eqa_absmax_slots + fused eqa_lift5_fft48k5_input_f16x2", fused_h), ("lift_conv_grouped + fft48k5_input_grouped", two), ("lift_conv_grouped alone", lift_only))
    for name, fn in (forms[2:3] if a.h2_only else forms):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name:>56}: {e0.elapsed_time(e1) / a.reps:7.3f} ms per launch  (B = {B}, {C} channels, {S} x {S})")
    raw = ctypes.CDLL(_lib.SO_PATH)
    if hasattr(raw, "eqa_debug_lf_clock"):
        # a clock build: [8 k .. 8 k + 7] the phases of the wave in slot k < 5, [64 .. 71] those of slot 5 (older builds: fewer slots),
        # [72 + k] the slot's row passes inside the sub-phases (older builds: 0), [40 + w] the HW_REG_HW_ID of wave w of block 0
        out = (ctypes.c_ulonglong * 128)()
        form = os.environ.get("EQA_LIFT_FFT_FORM", "h2")
        (fused_p if form == "bf16x3" else fused_h if form == "h2" else fused)()
        torch.cuda.synchronize()
        assert raw.eqa_debug_lf_clock(out) == 0
        names = ["stage + barrier 1", "prefetch issue", "role work", "barrier 2", "tail row passes", "barrier 3", "column read", "barrier 4"]
        items = max(1, (M * (C // 16) + 255) // 256) if M * (C // 16) >= 256 else 1
        hw = [out[40 + w] for w in range(12)]
        simd = {w: (hw[w] >> 4) & 3 for w in range(12)} if any(hw) else {}
        # [63]: 1 + EQA_LF_H2_DEAL of the h2 kernel (older builds: 0) -- from dealing 1 on wave 6 convolves; [62]: 1 + EQA_LF_H2_ROWDEAL
        # (older builds: 0) -- from row dealing 1 on column waves transform rows inside the sub-phases
        wave6 = "convolution wave 6" if form == "h2" and out[63] >= 2 else "row-transform wave 6"
        if form == "h2" and out[62]:
            print(f"EQA_LF_H2_DEAL = {out[63] - 1}, EQA_LF_H2_ROWDEAL = {out[62] - 1}")
        for k, (base, w, who) in enumerate(((0, 8, "convolution wave 8"), (8, 1, "column wave 1"), (16, 0, "column wave 0 (packed)"),
                                            (24, 6, wave6), (32, 11, "convolution wave 11"), (64, 2, "column wave 2"))):
            # [80 + 2 k], [81 + 2 k]: role work and barrier 2 of sub-phase 0 alone (h2; older builds: 0, there [base + 2], [base + 3] hold all four)
            sub0 = out[80 + 2 * k] + out[81 + 2 * k]
            tot = sum(out[base:base + 8]) + out[72 + k] + sub0
            if tot == 0:
                continue
            at = f" [SIMD {simd[w]}]" if simd else ""
            rows = f" | row passes in the sub-phases: {out[72 + k] // items}" if form == "h2" and w < 6 and out[62] else ""
            if form == "h2" and sub0:
                rows += f" | sub-phase 0 (not in the two figures above): role work {out[80 + 2 * k] // items}, barrier 2 {out[81 + 2 * k] // items}"
            print(f"{who}{at}: cycles per item (block 0, {items} items): " + " | ".join(f"{n}: {out[base + i] // items}" for i, n in enumerate(names))
                  + rows + f" | total {tot // items}")
        if simd:
            print("block 0, HW_REG_HW_ID per wave: " + " ".join(f"w{w}:0x{hw[w]:x}(simd {simd[w]}, wave slot {hw[w] & 15}, cu {(hw[w] >> 8) & 15})" for w in range(12)))

if __name__ == "__main__":
    main()
