#!/usr/bin/env python3
"""Cost of FreeU on one MI355X, on the bench workload: SD-1.5-size UNet (random init, bf16) + rank-4 LoRA,
256^2 px (32 x 32 latents), B = 32 slices, 50-step DDIM, hipGraph.  Variants: FreeU off and FreeU on with the SD-1.5 values of the
diffusers docs, (s1, s2, b1, b2) = (0.9, 0.2, 1.5, 1.6).  In ONE process every variant is warmed up with a 2-step run (which plans the
workspace and captures its step graph) and a full run, then the variants are timed in alternation (R rounds, device events around
each whole 50-step run).  Also reported: the profiled launches per step of both variants and the FreeU kernel's time per launch
(libmrisr's per-launch profiler: device events around each launch of eager steps), and the UNet's workspace bytes in both states.
Writes profiles/freeu_bench.json.

    timeout -k 10 600 python tools/bench_freeu.py --repeats 3
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
VARIANTS = {"off": None, "freeu": (0.9, 0.2, 1.5, 1.6)}


def log(msg):
    print(f"[bench_freeu +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per variant, taken in alternation")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--latent", type=int, default=32, help="latent h = w (256^2 px)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu_bench.json"))
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
    lat = torch.empty_like(x_T)
    lib = L.lib()

    def select(k):
        if VARIANTS[k] is None:
            unet.disable_freeu()
        else:
            unet.enable_freeu(*VARIANTS[k])

    # the variants share one UNet handle, whose workspace is planned per FreeU state: every switch re-plans and captures again, so each
    # timed run is preceded by an untimed 2-step run of the same variant (the plan and the capture), as the warm-up is
    samplers = {k: mrisr.Sampler(unet, sched, kind="ddim") for k in VARIANTS}
    finals, times, workspace = {}, {k: [] for k in VARIANTS}, {}

    def prepare(k):
        select(k)
        s = samplers[k]
        s.set_range(0, args.warmup_steps)
        lat.copy_(x_T)
        s.run(lat, ctx)
        torch.cuda.synchronize()
        s.set_range(0, n)

    for k in VARIANTS:
        prepare(k)
        lat.copy_(x_T)
        samplers[k].run(lat, ctx)
        torch.cuda.synchronize()
        finals[k] = lat.clone()
        workspace[k] = unet.workspace_bytes
        log(f"{k}: warmed up")
    for _ in range(args.repeats):
        for k in VARIANTS:
            prepare(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            samplers[k].run(lat, ctx)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))

    def profiled(k, steps=4):
        """device events around every launch of `steps` eager steps: launches per step, and the FreeU kernel's own class"""
        select(k)
        lib.mrisr_prof_reset()
        s = mrisr.Sampler(unet, sched, kind="ddim")
        s.set_range(0, 1)  # the per-run work (context projections, time-embedding table) outside the count
        lat.copy_(x_T)
        s.run(lat, ctx, use_graph=False)
        torch.cuda.synchronize()

        def count(first, last):
            lib.mrisr_prof_reset()
            lib.mrisr_prof_enable(1)
            s.set_range(first, last)
            lat.copy_(x_T)
            s.run(lat, ctx, use_graph=False)
            torch.cuda.synchronize()
            lib.mrisr_prof_enable(0)
            buf = C.create_string_buffer(1 << 20)
            got = lib.mrisr_prof_report(buf, len(buf))
            lib.mrisr_prof_reset()
            return json.loads(buf.value.decode()) if got > 0 else {}

        one, many = count(0, 1), count(0, 1 + steps)  # the difference: `steps` steps without the per-run launches
        total = lambda c: sum(v["launches"] for v in c.values())  # noqa: E731
        res = {"launches_per_step": (total(many) - total(one)) / steps}
        c = many.get("freeu")
        if c:
            res["freeu_launches_per_step"] = (c["launches"] - one.get("freeu", {"launches": 0})["launches"]) / steps
            res["freeu_us_per_launch"] = 1e3 * c["ms"] / c["launches"]
            res["freeu_bytes_per_launch"] = c["bytes"] / c["launches"]
        return res

    out = {"workload": f"SD-1.5-size UNet ({args.dtype}, random init) + rank-4 LoRA, {hw} x {hw} latents, B = {B} slices, {n}-step DDIM, "
                       f"hipGraph; variants timed in alternation after an untimed {args.warmup_steps}-step run of the same variant (plan + "
                       "capture), device events around each whole run",
           "batch": B, "latent": hw, "ddim_steps": n, "repeats": args.repeats, "dtype": args.dtype, "commit": commit_hash(), "variants": {}}
    base = statistics.median(times["off"])
    for k in VARIANTS:
        ms = statistics.median(times[k])
        out["variants"][k] = {"freeu": list(VARIANTS[k]) if VARIANTS[k] else None, "ms_per_run": ms, "ms_per_run_all": times[k],
                              "ms_per_step": ms / n, "slices_per_s": B / (ms * 1e-3), "cost_vs_off": ms / base,
                              "workspace_bytes": workspace[k], "finite": bool(torch.isfinite(finals[k]).all())}
        out["variants"][k].update(profiled(k))
        log(f"{k}: {ms / n:.3f} ms per step, {ms / base:.4f} x off, {out['variants'][k]['launches_per_step']} profiled launches per step")
    unet.disable_freeu()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
