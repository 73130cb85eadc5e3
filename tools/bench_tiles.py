#!/usr/bin/env python3
"""Cost of tiled sampling on one MI355X: SD-1.5-size UNet (random init, bf16) + rank-4 LoRA, a 64 x 64-latent
canvas (512^2 px) at B = 8 slices, 10-step DDIM, hipGraph.  Variants: direct (no tiles) and tile 32 with overlap 0 (T = 4), 8 and 16
(T = 9 each), Gaussian window.  In ONE process every variant is warmed up with a 2-step run (which captures its step graph), then the
variants are timed in alternation (R rounds, device events around each whole 10-step run).  Reported per variant: ms per step,
canvas slices/s, forward rows, the gather and the blend kernel's time per step (libmrisr's per-launch profiler: device events
around each launch of eager steps) and the relative L2 of the final latents against the direct run from the same x_T - information
only: a tiled run is a different sample, and the weights are random.  Writes profiles/tiles_bench.json.

    timeout -k 10 600 python tools/bench_tiles.py --repeats 3
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
VARIANTS = [None, (32, 0), (32, 8), (32, 16)]  # (tile, overlap) in latent pixels; None = direct


def log(msg):
    print(f"[bench_tiles +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def name_of(v):
    return "direct" if v is None else f"tile{v[0]}_overlap{v[1]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per variant, taken in alternation")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--canvas", type=int, default=64, help="latent h = w of the canvas")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=10)
    ap.add_argument("--warmup-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_bench.json"))
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
    B, hw, n = args.batch, args.canvas, args.ddim_steps
    g = torch.Generator(device=dev).manual_seed(SEED + 7)
    x_T = torch.randn((B, 4, hw, hw), device=dev, generator=g).contiguous()
    ctx = torch.randn((B, 77, cfg.cross_attention_dim), device=dev, generator=g)
    lat = torch.empty_like(x_T)
    lib = L.lib()

    def sampler_for(v):
        s = mrisr.Sampler(unet, sched, kind="ddim")
        if v is not None:
            s.set_tiles(v[0], v[1], "gaussian")
        return s

    samplers = {v: sampler_for(v) for v in VARIANTS}
    finals, times = {}, {v: [] for v in VARIANTS}
    for v in VARIANTS:
        s = samplers[v]
        s.set_range(0, args.warmup_steps)
        lat.copy_(x_T)
        s.run(lat, ctx)
        torch.cuda.synchronize()
        s.set_range(0, n)
        lat.copy_(x_T)
        s.run(lat, ctx)
        torch.cuda.synchronize()
        finals[v] = lat.clone()
        log(f"{name_of(v)}: warmed up ({s.tile_rows(B, hw, hw)} forward rows)")
    for _ in range(args.repeats):
        for v in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            samplers[v].run(lat, ctx)
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1))

    def kernel_ms(v, steps=4):
        """per-step time of the gather and the blend: device events around every launch of `steps` eager steps"""
        lib.mrisr_prof_reset()
        lib.mrisr_prof_enable(1)
        s = sampler_for(v)
        s.set_range(0, steps)
        lat.copy_(x_T)
        s.run(lat, ctx, use_graph=False)
        torch.cuda.synchronize()
        lib.mrisr_prof_enable(0)
        buf = C.create_string_buffer(1 << 20)
        k = lib.mrisr_prof_report(buf, len(buf))
        classes = json.loads(buf.value.decode()) if k > 0 else {}
        lib.mrisr_prof_reset()
        return {c: classes[c]["ms"] / max(1, classes[c]["launches"]) for c in ("tile_gather", "tile_blend") if c in classes}

    out = {"workload": f"SD-1.5-size UNet ({args.dtype}, random init) + rank-4 LoRA, {hw} x {hw}-latent canvas, B = {B} slices, "
                       f"{n}-step DDIM after a {args.warmup_steps}-step warm-up run, hipGraph; variants timed in alternation, device events "
                       "around each whole run; gaussian window",
           "note": "rel_l2_vs_direct is information only: a tiled run is a different sample, and the weights are random",
           "batch": B, "canvas": hw, "ddim_steps": n, "repeats": args.repeats, "dtype": args.dtype, "commit": commit_hash(), "variants": {}}
    base = finals[None].double()
    for v in VARIANTS:
        ms = statistics.median(times[v])
        rows = samplers[v].tile_rows(B, hw, hw)
        res = {"tile": v[0] if v else None, "overlap": v[1] if v else None, "tiles_per_slice": rows // B, "forward_rows": rows,
               "ms_per_run": ms, "ms_per_run_all": times[v], "ms_per_step": ms / n, "canvas_slices_per_s": B / (ms * 1e-3),
               "finite": bool(torch.isfinite(finals[v]).all()),
               "rel_l2_vs_direct": float((finals[v].double() - base).norm() / base.norm())}
        if v is not None:
            km = kernel_ms(v)
            res["gather_ms_per_step"], res["blend_ms_per_step"] = km.get("tile_gather"), km.get("tile_blend")
            tile_bytes = rows * 4 * v[0] * v[0] * 4
            res["gather_bytes_per_step"] = 2 * tile_bytes
            res["blend_bytes_per_step"] = tile_bytes + B * 4 * hw * hw * 4
        out["variants"][name_of(v)] = res
        log(f"{name_of(v)}: {res['ms_per_step']:.2f} ms per step, {res['canvas_slices_per_s']:.2f} canvas slices/s, {rows} forward rows, "
            f"gather {res.get('gather_ms_per_step')} ms blend {res.get('blend_ms_per_step')} ms, rel L2 vs direct {res['rel_l2_vs_direct']:.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
