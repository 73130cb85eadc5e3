#!/usr/bin/env python3
"""The 50-step DDIM bench workload (bench.py's batch, hipGraph, no feature cache) by LoRA rank, un-merged, and rank 64 merged as the
floor an un-merged adapter cannot beat.  One model at a time; device events around each whole run.

  python tools/bench_lora_rank.py [--ranks 4 16 32 64] [--repeats 3] [--out profiles/lora_rank_sampling.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[4, 16, 32, 64])
    ap.add_argument("--merged-rank", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=bench.B_PER_GPU)
    ap.add_argument("--ddim-steps", type=int, default=bench.N_DDIM)
    ap.add_argument("--lora-ff", action="store_true", help="adapters on ff.net.0.proj / ff.net.2 as well")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import mrisr
    from mrisr import params as P
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = mrisr.UNetConfig()
    base = P.random_state_dict(P.unet_param_shapes(cfg), bench.SEED, dev)
    sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sched.set_timesteps(args.ddim_steps)
    B = args.batch
    lr_lat, ctx, noise, _ = bench.synthetic_batch(B, dev, 0)
    a_T = float(sched.alphas_cumprod[int(sched.timesteps[0])])
    x_T = (lr_lat + (1 - a_T) ** 0.5 * noise).contiguous()
    lat = torch.empty_like(x_T)
    rows = []
    for r, fused in [(r, True) for r in args.ranks] + [(args.merged_rank, False)]:
        mrisr.check_lora_rank(r)
        sd = dict(base)
        sd.update(P.random_state_dict(P.lora_param_shapes(cfg, r), bench.SEED + 3, dev))
        if args.lora_ff:
            sd.update(P.random_state_dict(P.lora_ff_param_shapes(cfg, r), bench.SEED + 4, dev))
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=r, lora_alpha=r, lora_fused=fused, flash_attention=True)
        unet.load_state_dict(sd)
        s = mrisr.Sampler(unet, sched, kind="ddim")
        ms = []
        for i in range(args.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            s.run(lat, ctx)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms[1:])  # the first run plans, tunes and captures
        rows.append({"rank": r, "fused": fused, "ms_per_run": round(med, 2), "ms_per_step": round(med / args.ddim_steps, 3),
                     "slices_per_s": round(B / (med * 1e-3), 2), "finite": bool(torch.isfinite(lat).all())})
        print(json.dumps(rows[-1]), flush=True)
        del s, unet
    out = {"workload": f"bench.py's batch: SD-1.5-size UNet (bf16) + LoRA, 4x32x32 latents, {args.ddim_steps}-step DDIM, hipGraph, B = {B}",
           "lora_ff": bool(args.lora_ff), "repeats": args.repeats, "rows": rows}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
