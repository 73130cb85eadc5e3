#!/usr/bin/env python3
"""Cost and deviation of the sampler's feature cache on the bench workload: bench.py's own batch - SD-1.5-size
bf16 UNet + rank-4 LoRA, 256^2 slices (4x32x32 latents), B = 32, 50-step DDIM, hipGraph.  In ONE process it builds one sampler per
variant - uncached, interval {2, 3} x depth {1, 2, 3}, interval 5 / depth 1 - warms every one up, then times them in alternation
(R rounds over all variants, device events around each whole 50-step run) and reports per variant: slices/s (median over the
rounds), the kernel launches of a full and of a shallow step (libmrisr's per-launch profiler over eager steps) and the relative L2
of the final latents against the uncached run from the same x_T.  The weights are random, so that last figure is a numerics figure
only: it says how far the cached arithmetic moves the result, nothing about image quality.  Writes profiles/deepcache_bench.json.

    timeout -k 10 600 python tools/bench_cache.py --repeats 3
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

import bench  # noqa: E402  (the workload: bench.synthetic_batch, bench.SEED)

T_START = time.perf_counter()
VARIANTS = [(1, 1), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3), (5, 1)]  # (interval, depth); interval 1 = uncached


def log(msg):
    print(f"[bench_cache +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def name_of(v):
    return "uncached" if v[0] == 1 else f"interval{v[0]}_depth{v[1]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per variant (>= 3), taken in alternation")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=bench.B_PER_GPU)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=bench.N_DDIM)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepcache_bench.json"))
    args = ap.parse_args()

    import mrisr
    from mrisr import _lib as L
    from mrisr import params as P
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    log("init weights on device")
    cfg = mrisr.UNetConfig()
    sd = P.random_state_dict(P.unet_param_shapes(cfg), bench.SEED, dev)
    sd.update(P.random_state_dict(P.lora_param_shapes(cfg, 4), bench.SEED + 3, dev))
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype=args.dtype, lora_rank=4, lora_alpha=4, lora_fused=True, flash_attention=True)
    unet.load_state_dict(sd)
    torch.cuda.synchronize()
    log("weights packed")
    sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sched.set_timesteps(args.ddim_steps)
    B = args.batch
    lr_lat, ctx, noise, _ = bench.synthetic_batch(B, dev, 0)
    a_T = float(sched.alphas_cumprod[int(sched.timesteps[0])])
    x_T = (lr_lat + (1 - a_T) ** 0.5 * noise).contiguous()
    lat = torch.empty_like(x_T)
    lib = L.lib()

    def sampler_for(v):
        s = mrisr.Sampler(unet, sched, kind="ddim")
        if v[0] > 1:
            s.set_cache(*v)
        return s

    samplers = {v: sampler_for(v) for v in VARIANTS}
    finals, times = {}, {v: [] for v in VARIANTS}
    for v in VARIANTS:
        for _ in range(max(1, args.warmup)):
            lat.copy_(x_T)
            samplers[v].run(lat, ctx)
            torch.cuda.synchronize()
        finals[v] = lat.clone()
        log(f"{name_of(v)}: warmed up")
    for r in range(args.repeats):
        for v in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            samplers[v].run(lat, ctx)
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1))

    def launches(v, last):
        """kernel launches of eager steps [0, last) of variant v"""
        lib.mrisr_prof_reset()
        lib.mrisr_prof_enable(1)
        s = sampler_for(v)
        s.set_range(0, last)
        lat.copy_(x_T)
        s.run(lat, ctx, use_graph=False)
        torch.cuda.synchronize()
        lib.mrisr_prof_enable(0)
        buf = C.create_string_buffer(1 << 20)
        n = lib.mrisr_prof_report(buf, len(buf))
        classes = json.loads(buf.value.decode()) if n > 0 else {}
        lib.mrisr_prof_reset()
        return sum(c["launches"] for c in classes.values())

    out = {"workload": f"bench.py's batch: SD-1.5-size UNet ({args.dtype}) + rank-4 LoRA, 4x32x32 latents, {args.ddim_steps}-step DDIM, "
                       f"hipGraph, B = {B} slices; variants timed in alternation, device events around each whole run",
           "note": "random weights: rel_l2_vs_uncached is a numerics figure only, not image quality",
           "batch": B, "ddim_steps": args.ddim_steps, "repeats": args.repeats, "warmup": args.warmup, "dtype": args.dtype,
           "commit": commit_hash(), "variants": {}}
    full_launches = launches((1, 1), 1)
    base_ms = statistics.median(times[(1, 1)])
    for v in VARIANTS:
        ms = statistics.median(times[v])
        n_full = sum(1 for i in range(args.ddim_steps) if i % v[0] == 0)
        res = {"interval": v[0], "depth": v[1], "ms_per_run": ms, "ms_per_run_all": times[v], "slices_per_s": B / (ms * 1e-3),
               "speedup_vs_uncached": base_ms / ms, "full_steps": n_full, "shallow_steps": args.ddim_steps - n_full,
               "launches_full_step": full_launches, "finite": bool(torch.isfinite(finals[v]).all()),
               "rel_l2_vs_uncached": float((finals[v].double() - finals[(1, 1)].double()).norm() / finals[(1, 1)].double().norm())}
        if v[0] > 1:
            res["launches_full_step"] = launches(v, 1)  # (+ one device-to-device copy node, which is not a kernel)
            res["launches_shallow_step"] = launches(v, 2) - res["launches_full_step"]
        out["variants"][name_of(v)] = res
        log(f"{name_of(v)}: {ms:.1f} ms per run, {res['slices_per_s']:.1f} slices/s ({res['speedup_vs_uncached']:.2f}x), "
            f"launches full {res['launches_full_step']} shallow {res.get('launches_shallow_step')}, rel L2 vs uncached {res['rel_l2_vs_uncached']:.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
