#!/usr/bin/env python3
"""Cost of low-frequency consistency on one MI355X, on the workload of bench.py: SD-1.5-size UNet with rank-4 LoRA
(random init, bf16), 256^2 px (32 x 32 latents), B = 32 slices, 50-step DDIM, hipGraph.  Variants:

    plain       the run without the keywords - the launches and the bits of the parent commit
    bilinear    consistency_ref = the LR latents, factor 4, weight 1 on every step, the bilinear filter: one more launch per step
    nearest     the same with the nearest filter
    zero        the bilinear run with weight 0: the launch is there and returns at once; must end in the bits of ``plain``

In ONE process every variant is warmed up with a 2-step run (which captures its step graph) and a full run, then the variants are timed
in alternation (R rounds, device events around each whole 50-step run).  Reported per variant: the median ms per run, its ratio to
``plain`` beside the spread of ``plain`` itself, the cost per launch inside the graph ((ms - ms of plain) / steps) and the kernel's own
time per launch from libmrisr's per-launch profiler over eager steps.  Writes profiles/consistency_bench.json.

    timeout -k 10 600 python tools/bench_consistency.py --repeats 5
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MRISR_TUNE_CACHE", os.path.join(ROOT, "profiles", "r03_tune_cache.tsv"))
for p in (ROOT, os.path.join(ROOT, "mri-diffusion-superresolution_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SEED = 20260501
T_START = time.perf_counter()


def log(msg):
    print(f"[bench_consistency +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="timed runs per variant, taken in alternation")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--latent", type=int, default=32, help="latent h = w (256^2 px)")
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.json"))
    args = ap.parse_args()

    import mrisr
    from mrisr import _lib as L
    from mrisr import params as P
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    log("init weights on device")
    cfg = mrisr.UNetConfig()
    sd = P.random_state_dict(P.unet_param_shapes(cfg), SEED, dev)
    sd.update(P.random_state_dict(P.lora_param_shapes(cfg, 4), SEED + 3, dev))
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype=args.dtype, lora_rank=4, lora_alpha=4, lora_fused=True, flash_attention=True)
    unet.load_state_dict(sd)
    torch.cuda.synchronize()
    log("weights packed")
    sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sched.set_timesteps(args.ddim_steps)
    B, hw, n = args.batch, args.latent, args.ddim_steps
    g = torch.Generator(device=dev).manual_seed(SEED + 7)
    x_T = torch.randn((B, 4, hw, hw), device=dev, generator=g).contiguous()
    ctx = torch.randn((B, 77, cfg.cross_attention_dim), device=dev, generator=g)
    # a smooth field at the scale of VAE latents stands in for the LR latents
    ref = (0.18215 * torch.nn.functional.interpolate(torch.randn((B, 4, hw // 8, hw // 8), device=dev, generator=g), size=(hw, hw),
                                                     mode="bicubic", align_corners=False)).contiguous()
    lat = torch.empty_like(x_T)
    lib = L.lib()
    on = dict(consistency_ref=ref, consistency_factor=args.factor)
    variants = {"plain": dict(), "bilinear": dict(on), "nearest": dict(on, consistency_filter="nearest"),
                "zero": dict(on, consistency_weight=0.0)}
    samplers = {k: mrisr.Sampler(unet, sched, kind="ddim") for k in variants}
    finals, times = {}, {k: [] for k in variants}

    def run(s, k, **more):
        s.run(lat, ctx, **variants[k], **more)

    for k in variants:
        s = samplers[k]
        s.set_range(0, args.warmup_steps)
        lat.copy_(x_T)
        run(s, k)
        s.set_range(0, n)
        lat.copy_(x_T)
        run(s, k)
        torch.cuda.synchronize()
        finals[k] = lat.clone()
        log(f"{k}: warmed up")
    for _ in range(args.repeats):
        for k in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            run(samplers[k], k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))

    def launches(k, steps=4):
        """what libmrisr's per-launch profiler sees over `steps` eager steps: launches per step, and the consistency kernel's own time"""
        lib.mrisr_prof_reset()
        lib.mrisr_prof_enable(1)
        s = mrisr.Sampler(unet, sched, kind="ddim")
        s.set_range(0, steps)
        lat.copy_(x_T)
        run(s, k, use_graph=False)
        torch.cuda.synchronize()
        lib.mrisr_prof_enable(0)
        buf = C.create_string_buffer(1 << 20)
        m = lib.mrisr_prof_report(buf, len(buf))
        classes = json.loads(buf.value.decode()) if m > 0 else {}
        lib.mrisr_prof_reset()
        out = {"profiled_launches_per_step": sum(c["launches"] for c in classes.values()) / steps}
        if "consistency" in classes:
            c = classes["consistency"]
            out["consistency"] = {"launches_per_step": c["launches"] / steps, "us_per_launch_eager": 1e3 * c["ms"] / c["launches"]}
        return out

    plain = statistics.median(times["plain"])
    out = {"workload": f"SD-1.5-size UNet + rank-4 LoRA ({args.dtype}, random init), {hw} x {hw} latents, B = {B} slices, {n}-step DDIM, hipGraph, "
                       f"consistency factor {args.factor}; variants timed in alternation after a {args.warmup_steps}-step and a full warm-up run, "
                       "device events around each whole run",
           "batch": B, "latent": hw, "ddim_steps": n, "factor": args.factor, "repeats": args.repeats, "dtype": args.dtype,
           "commit": commit_hash(), "spread_of_plain": (max(times["plain"]) - min(times["plain"])) / plain, "variants": {}}
    for k in variants:
        ms = statistics.median(times[k])
        out["variants"][k] = {"ms_per_run": ms, "ms_per_run_all": times[k], "ratio_to_plain": ms / plain,
                              "us_per_launch_in_graph": 1e3 * (ms - plain) / n if k != "plain" else None,
                              "same_bits_as_plain": bool(torch.equal(finals[k], finals["plain"])),
                              "finite": bool(torch.isfinite(finals[k]).all()), "launches": launches(k)}
        log(f"{k}: {ms:.2f} ms per run, {ms / plain:.4f} x plain, {out['variants'][k]}")
    assert out["variants"]["zero"]["same_bits_as_plain"] and not out["variants"]["bilinear"]["same_bits_as_plain"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
