#!/usr/bin/env python3
"""Per-step cost of the multistep sampler kinds on the flagship workload: SD-1.5-size bf16 UNet + rank-4 LoRA, 256^2 slices
(4x32x32 latents), 50 steps, hipGraph, B = 32 slices.  In ONE process and in this order it times kind="ddim", "unipc" (order 2) and
"dpmsolver++" (order 2) on the same timestep grid with bench.py's scheme (W warm-up batches, then K timed batches between two
fences), then reads the step kernel's own time from libmrisr's per-launch profiler over two eager steps.  Writes
profiles/multistep_bench.json.

    timeout -k 10 600 python tools/bench_multistep.py --steps 3 --warmup 1
"""
import argparse
import ctypes as C
import json
import os
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
LATENT = 32
N_DDIM = 50
T_START = time.perf_counter()


def log(msg):
    print(f"[bench_multistep +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed batches per leg")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=N_DDIM)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistep_bench.json"))
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
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(SEED)
    x_T = torch.randn((B, 4, LATENT, LATENT), device=dev, generator=g)
    ctx = torch.randn((B, 77, 768), device=dev, generator=g)
    lat = torch.empty_like(x_T)
    lib = L.lib()

    def leg(name, kind):
        sampler = mrisr.Sampler(unet, sched, kind=kind)

        def one_batch():
            lat.copy_(x_T)
            sampler.run(lat, ctx)

        for _ in range(args.warmup):
            one_batch()
            torch.cuda.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one_batch()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        finite = bool(torch.isfinite(lat).all())
        lib.mrisr_prof_reset()
        lib.mrisr_prof_enable(1)
        s2 = mrisr.Sampler(unet, sched, kind=kind)
        s2.set_range(0, 2)
        lat.copy_(x_T)
        s2.run(lat, ctx, use_graph=False)
        torch.cuda.synchronize()
        lib.mrisr_prof_enable(0)
        buf = C.create_string_buffer(1 << 20)
        n = lib.mrisr_prof_report(buf, len(buf))
        classes = json.loads(buf.value.decode()) if n > 0 else {}
        lib.mrisr_prof_reset()
        ms_step = elapsed / args.steps / args.ddim_steps * 1e3
        res = {"ms_per_denoising_step": ms_step, "slices_per_s": B * args.steps / elapsed, "finite": finite,
               "launches_per_step": sum(v["launches"] for v in classes.values()) / 2,
               "sampler_step_kernel_us": classes.get("sampler_step", {}).get("ms", 0.0) / 2 * 1e3}
        log(f"{name}: {ms_step:.3f} ms per denoising step, step kernel {res['sampler_step_kernel_us']:.1f} us, "
            f"{res['launches_per_step']:.0f} profiled launches per step")
        return res

    out = {"workload": f"SD-1.5-size UNet ({args.dtype}) + rank-4 LoRA, 4x{LATENT}x{LATENT} latents, {args.ddim_steps} steps, hipGraph, "
                       f"B = {B} slices; one UNet forward + one fused step kernel per step for every kind",
           "batch": B, "ddim_steps": args.ddim_steps, "steps": args.steps, "warmup": args.warmup, "dtype": args.dtype,
           "commit": commit_hash()}
    for kind in ("ddim", "unipc", "dpmsolver++"):
        out[kind] = leg(kind, kind)
    base = out["ddim"]["ms_per_denoising_step"]
    out["ratio_over_ddim"] = {k: out[k]["ms_per_denoising_step"] / base for k in ("unipc", "dpmsolver++")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
