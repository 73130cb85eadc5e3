#!/usr/bin/env python3
"""Kernel time of the LoRA weight gradients by rank: `lora_wgrad` (ranks 4 .. 16, the streaming VALU kernel, f32 Q)
against `lora_wgrad_hr` (ranks 32 .. 128, bf16 MFMA through transposed LDS reads, bf16 Q), from the per-launch HIP-event profiler, the
median of --reps launches.  Shapes: the dB / dA pair of the fused QKV projection of level 0 at bs = 32 (M = 32768, C = 320, three modules).

  python tools/bench_lora_wgrad.py [--rows 32768] [--width 320] [--reps 7] [--out profiles/lora_highrank_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mrisr import _lib as L
    from mrisr import ops
    lib = L.lib()
    M, W, nmod = args.rows, args.width, 3
    g = torch.Generator(device="cuda").manual_seed(18)
    dY = torch.randn((M, nmod * W), generator=g, device="cuda").bfloat16()
    x = torch.randn((M, W), generator=g, device="cuda").bfloat16()

    def timed(name, fn):
        ms = []
        for _ in range(args.reps + 1):
            lib.mrisr_prof_reset(); lib.mrisr_prof_enable(1)
            fn()
            torch.cuda.synchronize()
            lib.mrisr_prof_enable(0)
            buf = C.create_string_buffer(1 << 20)
            n = lib.mrisr_prof_report(buf, len(buf))
            ms.append(json.loads(buf.value[:n].decode())[name]["ms"])
        lib.mrisr_prof_reset()
        return round(statistics.median(ms[1:]), 4)  # the first launch pays for the code object

    rows = []
    for r in (4, 8, 16, 32, 64, 128):
        hr = r > 16
        rp = (r + 63) // 64 * 64 if hr else r
        q = torch.randn((M, nmod * rp), generator=g, device="cuda")
        q = q.bfloat16() if hr else q
        oB = [torch.zeros((W, r), device="cuda") for _ in range(nmod)]
        oA = [torch.zeros((r, W), device="cuda") for _ in range(nmod)]
        op, name = (ops.lora_wgrad_hr, "lora_wgrad_hr") if hr else (ops.lora_wgrad, "lora_wgrad")
        dB = timed(name, lambda: op(dY, q, M, nmod * W, 0, r, nmod, W, oB))
        dA = timed(name, lambda: op(x, q, M, W, 1, r, nmod, W, oA))
        read_ms = lambda nbytes: nbytes / 8e12 * 1e3  # 8 TB/s HBM3E peak
        rows.append({"rank": r, "kernel": name, "dB_ms": dB, "dA_ms": dA, "dB_GFLOP": round(2e-9 * M * nmod * W * r, 2),
                     "dA_GFLOP": round(2e-9 * M * W * nmod * r, 2), "dB_read_floor_ms": round(read_ms(dY.numel() * 2 + q.numel() * q.element_size()), 4),
                     "dA_read_floor_ms": round(read_ms(x.numel() * 2 + q.numel() * q.element_size()), 4)})
        print(json.dumps(rows[-1]), flush=True)
    out = {"metric": "lora_wgrad_kernel_ms_by_rank", "rows": M, "width": W, "modules": nmod, "dtype": "bf16", "reps": args.reps, "ranks": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
