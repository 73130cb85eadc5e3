#!/usr/bin/env python3
"""What ``Sampler.run(skip_neutral=True)`` saves on one MI355X, on the bench workload: SD-1.5-size UNet + rank-4 LoRA
(random init, bf16), 256^2 px (32 x 32 latents), B = 32 slices, 50-step DDIM, hipGraph.  Pairs, each timed with the option off and on:

    plain / -        the unguided run (B rows per step): what a guided step is measured against
    cfg              classifier-free guidance (g = 3) with guidance_interval = (0.2, 0.8): 30 guided steps, 20 neutral ones
    cnet             a ControlNet with control_guidance_end = 0.5: 25 steps with the ControlNet, 25 with scale 0

In ONE process every variant is warmed up (an untimed short run - the plan and the captures - and a full run), then the variants are
timed in alternation (R rounds, device events around each whole 50-step run).  Reported per variant: ms per run, the library's own
``last_run_stats``, and for the skipping runs the ratio to their skip-off twin, the relative L2 distance of the final latents from the
twin's (rounding on the skipped steps) and the saving the row count predicts: the skipped share of the rows times the measured
difference between a guided and a plain step.  Writes profiles/skip_bench.json.

    timeout -k 10 900 python tools/bench_skip.py --repeats 3
"""
import argparse
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

SEED = 20260701
T_START = time.perf_counter()


def log(msg):
    print(f"[bench_skip +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


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
    ap.add_argument("--no-controlnet", action="store_true", help="leave the ControlNet pair out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_bench.json"))
    args = ap.parse_args()

    import mrisr
    from mrisr import params as P
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    log("init weights on device")
    cfg = mrisr.UNetConfig()
    sd = P.random_state_dict(P.unet_param_shapes(cfg), SEED, dev)
    sd.update(P.random_state_dict(P.lora_param_shapes(cfg, 4), SEED + 3, dev))
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype=args.dtype, lora_rank=4, lora_alpha=4, lora_fused=True, flash_attention=True)
    unet.load_state_dict(sd)
    cnet = None
    if not args.no_controlnet:
        cnet = mrisr.ControlNetModel(cfg, compute_dtype=args.dtype, flash_attention=True)
        cnet.load_state_dict(P.random_state_dict(P.controlnet_param_shapes(cfg), SEED + 1, dev))
    torch.cuda.synchronize()
    log("weights packed")
    sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sched.set_timesteps(args.ddim_steps)
    B, hw, n = args.batch, args.latent, args.ddim_steps
    g = torch.Generator(device=dev).manual_seed(SEED + 7)
    x_T = torch.randn((B, 4, hw, hw), device=dev, generator=g).contiguous()
    ctx = torch.randn((B, 77, cfg.cross_attention_dim), device=dev, generator=g)
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), device=dev, generator=g)
    cond = torch.randn((B, 3, 8 * hw, 8 * hw), device=dev, generator=g)
    lat = torch.empty_like(x_T)
    cfg_kw = dict(uncond_hidden_states=ctx_u, guidance_scale=3.0)
    variants = {"plain": (None, dict()),
                "cfg_full": (None, dict(cfg_kw)),
                "cfg": (None, dict(cfg_kw, guidance_interval=(0.2, 0.8))),
                "cfg_skip": (None, dict(cfg_kw, guidance_interval=(0.2, 0.8), skip_neutral=True))}
    twin = {"cfg_skip": "cfg"}
    if cnet is not None:
        variants["cnet"] = (cnet, dict(controlnet_cond=cond, control_guidance_end=0.5))
        variants["cnet_skip"] = (cnet, dict(controlnet_cond=cond, control_guidance_end=0.5, skip_neutral=True))
        twin["cnet_skip"] = "cnet"
    # the variants share the model handles, whose workspaces are planned per (rows, table mode): a switch re-plans and captures again, so
    # each timed run is preceded by an untimed short run of the same variant
    samplers = {k: mrisr.Sampler(unet, sched, c, kind="ddim") for k, (c, _) in variants.items()}
    finals, stats, times = {}, {}, {k: [] for k in variants}

    def run(k):
        samplers[k].run(lat, ctx, **variants[k][1])

    # a skipping run captures one graph per step variant: its untimed run reaches the first step of every variant
    pattern = {"cfg_skip": mrisr.step_variants(mrisr.step_schedule(sched.timesteps, guidance_scale=3.0, guidance_interval=(0.2, 0.8)), None, 2),
               "cnet_skip": mrisr.step_variants(None, mrisr.conditioning_schedule(n, control_guidance_end=0.5), 1, True, 0)}
    warm = {k: max([args.warmup_steps] + [1 + pattern[k].index(v) for v in set(pattern.get(k, []))]) for k in variants}

    def prepare(k):
        """plan and capture outside the timed run (same first step: the same step plan)"""
        s = samplers[k]
        s.set_range(0, warm[k])
        lat.copy_(x_T)
        run(k)
        torch.cuda.synchronize()
        s.set_range(0, n)

    for k in variants:
        prepare(k)
        lat.copy_(x_T)
        run(k)
        torch.cuda.synchronize()
        finals[k], stats[k] = lat.clone(), samplers[k].last_run_stats
        log(f"{k}: warmed up, {stats[k]}")
    for _ in range(args.repeats):
        for k in variants:
            prepare(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            run(k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))

    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"workload": f"SD-1.5-size UNet + rank-4 LoRA ({args.dtype}, random init), {hw} x {hw} latents, B = {B} slices, {n}-step DDIM, hipGraph; "
                       "variants timed in alternation after untimed short runs of the same variant (plan + captures), device events around "
                       "each whole run",
           "batch": B, "latent": hw, "ddim_steps": n, "repeats": args.repeats, "dtype": args.dtype, "commit": commit_hash(), "variants": {}}
    for k in variants:
        v = {"ms_per_run": med[k], "ms_per_run_all": times[k], "ms_per_step": med[k] / n, "last_run_stats": stats[k],
             "spread": (max(times[k]) - min(times[k])) / med[k], "finite": bool(torch.isfinite(finals[k]).all())}
        if k in twin:
            t = twin[k]
            v["vs"] = t
            v["ratio"] = med[k] / med[t]
            v["rel_l2_to_twin"] = float((finals[k] - finals[t]).norm() / finals[t].norm())
        out["variants"][k] = v
    # the saving the row count predicts for cfg_skip: (skipped rows / B) steps' worth of (guided step - plain step)
    per_guided, per_plain = med["cfg_full"] / n, med["plain"] / n
    skipped_steps = (stats["cfg"]["unet_rows"] - stats["cfg_skip"]["unet_rows"]) / B
    out["cfg_skip_expected_saving_ms"] = skipped_steps * (per_guided - per_plain)
    out["cfg_skip_measured_saving_ms"] = med["cfg"] - med["cfg_skip"]
    for k, v in out["variants"].items():
        log(f"{k}: {v['ms_per_run']:.1f} ms per run (spread {v['spread']:.3%})" + (f", {v['ratio']:.4f} x {v['vs']}, rel L2 {v['rel_l2_to_twin']:.2e}" if "vs" in v else ""))
    log(f"cfg_skip saving: measured {out['cfg_skip_measured_saving_ms']:.1f} ms, predicted from rows {out['cfg_skip_expected_saving_ms']:.1f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
