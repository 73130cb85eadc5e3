#!/usr/bin/env python3
"""Cost of reading the guidance and FreeU strengths from the per-step schedule table on one MI355X, on the
bench workload: SD-1.5-size UNet (random init, bf16) + rank-4 LoRA, 256^2 px (32 x 32 latents), B = 32 slices, 50-step DDIM, hipGraph.
Pairs: a guided run (g = 2; and g = 2 with guidance_rescale 0.7) with scalars against the same run with a CONSTANT schedule, and a
plain run with FreeU on against the same run with the four values in the table.  In ONE process every variant is warmed up with a
2-step run (which captures its step graph) and a full run, then the variants are timed in alternation (R rounds, device events
around each whole 50-step run); the two runs of a pair must end in the same bits.  Also reported: the time per launch of the
guided step kernel (profiler scope ``sampler_step``) and of the FreeU launches (``freeu``) from libmrisr's per-launch profiler
(device events around each launch of eager steps).  Writes profiles/schedule_bench.json.

    timeout -k 10 900 python tools/bench_schedule.py --repeats 2
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED = 20260501
T_START = time.perf_counter()
FREEU = (0.9, 0.2, 1.5, 1.6)


def log(msg):
    print(f"[bench_schedule +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def constant(n, g=1.0, phi=0.0, freeu=(1.0, 1.0, 1.0, 1.0)):
    return np.tile(np.asarray((g, 0.0, phi) + tuple(freeu) + (0.0,), dtype=np.float32), (n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per variant, taken in alternation")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--latent", type=int, default=32, help="latent h = w (256^2 px)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schedule_bench.json"))
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
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), device=dev, generator=g)
    lat = torch.empty_like(x_T)
    lib = L.lib()
    cfg_kw = dict(uncond_hidden_states=ctx_u, guidance_scale=2.0)
    # name -> (run keywords, FreeU on the UNet); a pair is (<name>_scalar, <name>_table)
    variants = {"cfg_scalar": (dict(cfg_kw), False), "cfg_table": (dict(cfg_kw, schedule=constant(n, 2.0)), False),
                "cfg_rescale_scalar": (dict(cfg_kw, guidance_rescale=0.7), False),
                "cfg_rescale_table": (dict(cfg_kw, guidance_rescale=0.7, schedule=constant(n, 2.0, 0.7)), False),
                "freeu_scalar": ({}, True), "freeu_table": (dict(schedule=constant(n, freeu=FREEU)), True)}

    def run(s, k, **more):
        kw, freeu = variants[k]
        if freeu:
            unet.enable_freeu(*FREEU)
        try:
            s.run(lat, ctx, **kw, **more)
        finally:
            if freeu:
                unet.disable_freeu()

    # the variants share one UNet handle, whose workspace is planned per (rows, FreeU mode): a switch re-plans and captures again, so each
    # timed run is preceded by an untimed 2-step run of the same variant (the plan and the capture), as the warm-up is
    samplers = {k: mrisr.Sampler(unet, sched, kind="ddim") for k in variants}
    finals, times = {}, {k: [] for k in variants}

    def prepare(k):
        s = samplers[k]
        s.set_range(0, args.warmup_steps)
        lat.copy_(x_T)
        run(s, k)
        torch.cuda.synchronize()
        s.set_range(0, n)

    for k in variants:
        prepare(k)
        lat.copy_(x_T)
        run(samplers[k], k)
        torch.cuda.synchronize()
        finals[k] = lat.clone()
        log(f"{k}: warmed up")
    for _ in range(args.repeats):
        for k in variants:
            prepare(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            run(samplers[k], k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))

    def per_launch(k, steps=4):
        """device events around every launch of `steps` eager steps: us per launch of the guided step and of the FreeU launches"""
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
        return {c: {"launches": classes[c]["launches"], "us_per_launch": 1e3 * classes[c]["ms"] / classes[c]["launches"]}
                for c in ("sampler_step", "freeu") if c in classes}

    out = {"workload": f"SD-1.5-size UNet ({args.dtype}, random init) + rank-4 LoRA, {hw} x {hw} latents, B = {B} slices, {n}-step DDIM, "
                       f"hipGraph; variants timed in alternation after an untimed {args.warmup_steps}-step run of the same variant (plan + "
                       "capture), device events around each whole run; per-launch times from eager steps",
           "batch": B, "latent": hw, "ddim_steps": n, "repeats": args.repeats, "dtype": args.dtype, "commit": commit_hash(), "variants": {}}
    for k in variants:
        ms = statistics.median(times[k])
        pair = k.rsplit("_", 1)[0] + "_scalar"
        out["variants"][k] = {"ms_per_run": ms, "ms_per_run_all": times[k], "ms_per_step": ms / n,
                              "vs_scalar": ms / statistics.median(times[pair]), "same_bits_as_scalar": bool(torch.equal(finals[k], finals[pair])),
                              "finite": bool(torch.isfinite(finals[k]).all()), "per_launch": per_launch(k)}
        log(f"{k}: {ms:.1f} ms per run, {out['variants'][k]['vs_scalar']:.4f} x scalar, same bits {out['variants'][k]['same_bits_as_scalar']}, "
            f"{out['variants'][k]['per_launch']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
