#!/usr/bin/env python3
"""Cost of the conditioning table on one MI355X, on the ControlNet workload of BASELINE config 4: SD-1.5-size UNet
and ControlNet (random init, bf16), 512^2 px (64 x 64 latents), B = 16 slices, 50-step DDIM, hipGraph.  Pairs:

    plain       the run without the keywords - the launches and the bits of the parent commit: per residual a device-to-device copy out of
                the ControlNet and a scalar add_inplace in the UNet (the NHWC residual is read in place: no import copy)
    table       the same run with the constant table {1, 1}: the output convolutions write in place, two multi-tensor launches add
    cfg         classifier-free guidance (g = 2), the ControlNet on 2B rows
    cfg_guess   the same with guess_mode: the ControlNet on the B conditional rows

In ONE process every variant is warmed up with a 2-step run (which plans the workspaces and captures its step graph) and a full run, then
the variants are timed in alternation (R rounds, device events around each whole 50-step run).  ``table`` must end in the bits of
``plain``.  Also reported: the launches per step of each variant, counted by libmrisr's per-launch profiler over eager steps.  Writes
profiles/condctl_bench.json.

    timeout -k 10 900 python tools/bench_condctl.py --repeats 2
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

SEED = 20260601
T_START = time.perf_counter()


def log(msg):
    print(f"[bench_condctl +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per variant, taken in alternation")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=64, help="latent h = w (512^2 px)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "condctl_bench.json"))
    args = ap.parse_args()

    import mrisr
    from mrisr import _lib as L
    from mrisr import params as P
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    log("init weights on device")
    cfg = mrisr.UNetConfig()
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype=args.dtype, flash_attention=True)
    unet.load_state_dict(P.random_state_dict(P.unet_param_shapes(cfg), SEED, dev))
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
    lib = L.lib()
    neutral = np.tile(np.float32([1, 1, 0, 0]), (n, 1))
    cfg_kw = dict(uncond_hidden_states=ctx_u, guidance_scale=2.0)
    variants = {"plain": dict(), "table": dict(conditioning=neutral), "cfg": dict(cfg_kw), "cfg_guess": dict(cfg_kw, guess_mode=True)}
    pair_of = {"plain": "plain", "table": "plain", "cfg": "cfg", "cfg_guess": "cfg"}

    def run(s, k, **more):
        s.run(lat, ctx, controlnet_cond=cond, **variants[k], **more)

    # the variants share the model handles, whose workspaces are planned per (rows, table mode): a switch re-plans and captures again, so
    # each timed run is preceded by an untimed 2-step run of the same variant (the plan and the capture), as the warm-up is
    samplers = {k: mrisr.Sampler(unet, sched, cnet, kind="ddim") for k in variants}
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

    def launches(k, steps=2):
        """kernel launches per step that the library's profiler sees over `steps` eager steps (copies are not launches of its own)"""
        lib.mrisr_prof_reset()
        lib.mrisr_prof_enable(1)
        s = mrisr.Sampler(unet, sched, cnet, kind="ddim")
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
        if "cond_add" in classes:
            out["cond_add"] = {"launches_per_step": classes["cond_add"]["launches"] / steps,
                               "us_per_launch": 1e3 * classes["cond_add"]["ms"] / classes["cond_add"]["launches"]}
        return out

    out = {"workload": f"SD-1.5-size UNet + ControlNet ({args.dtype}, random init), {hw} x {hw} latents, B = {B} slices, {n}-step DDIM, hipGraph; "
                       f"variants timed in alternation after an untimed {args.warmup_steps}-step run of the same variant (plan + capture), "
                       "device events around each whole run",
           "batch": B, "latent": hw, "ddim_steps": n, "repeats": args.repeats, "dtype": args.dtype, "commit": commit_hash(), "variants": {}}
    for k in variants:
        ms, pair = statistics.median(times[k]), pair_of[k]
        ref = times[pair]
        out["variants"][k] = {"ms_per_run": ms, "ms_per_run_all": times[k], "ms_per_step": ms / n, "vs": pair,
                              "ratio": ms / statistics.median(ref), "spread_of_pair": (max(ref) - min(ref)) / statistics.median(ref),
                              "same_bits_as_pair": bool(torch.equal(finals[k], finals[pair])),
                              "finite": bool(torch.isfinite(finals[k]).all()), "launches": launches(k)}
        log(f"{k}: {ms:.1f} ms per run, {out['variants'][k]['ratio']:.4f} x {pair}, same bits {out['variants'][k]['same_bits_as_pair']}, "
            f"{out['variants'][k]['launches']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
