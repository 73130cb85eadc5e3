#!/usr/bin/env python3
"""Cost of perturbed-attention guidance on one MI355X, on the bench workload: SD-1.5-size UNet (random init,
bf16) + rank-4 LoRA, 256^2 px (32 x 32 latents), B = 32 slices, 50-step DDIM, hipGraph.  Variants: plain, classifier-free guidance
(g = 2: the 2B-row forward), PAG alone on ("mid",) and PAG alone on all 16 transformer blocks (both the 2B-row forward, minus the
attention launches of the perturbed rows).  In ONE process every variant is warmed up with a 2-step run (which captures its step
graph) and a full run, then the variants are timed in alternation (R rounds, device events around each whole 50-step run).
Also reported: the identity-attention kernel's time and achieved bytes per second at level 0 (PAG applied to
down_blocks.0.attentions.0 only, libmrisr's per-launch profiler: device events around each launch of eager steps), to be read against
``subpix_shuffle``'s copy rate in DESIGN.md section 7.  Writes profiles/pag_bench.json.

    timeout -k 10 900 python tools/bench_pag.py --repeats 2
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
ALL = ("down_blocks", "mid", "up_blocks")
VARIANTS = {"plain": {}, "cfg_g2": dict(guidance_scale=2.0), "pag_mid": dict(pag_scale=3.0, pag_applied_layers=("mid",)),
            "pag_all16": dict(pag_scale=3.0, pag_applied_layers=ALL)}


def log(msg):
    print(f"[bench_pag +{time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2, help="timed runs per variant, taken in alternation")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--latent", type=int, default=32, help="latent h = w (256^2 px)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--warmup-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pag_bench.json"))
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

    def run(s, kw, **more):
        """one run from x_T; classifier-free guidance gets its unconditional context"""
        extra = dict(uncond_hidden_states=ctx_u) if "guidance_scale" in kw else {}
        s.run(lat, ctx, **kw, **extra, **more)

    # the variants share one UNet handle, whose workspace is planned per (rows, PAG state): every switch re-plans and captures again, so
    # each timed run is preceded by an untimed 2-step run of the same variant (the plan and the capture), as the warm-up is
    samplers = {k: mrisr.Sampler(unet, sched, kind="ddim") for k in VARIANTS}
    finals, times = {}, {k: [] for k in VARIANTS}

    def prepare(k):
        s = samplers[k]
        s.set_range(0, args.warmup_steps)
        lat.copy_(x_T)
        run(s, VARIANTS[k])
        torch.cuda.synchronize()
        s.set_range(0, n)

    for k in VARIANTS:
        prepare(k)
        lat.copy_(x_T)
        run(samplers[k], VARIANTS[k])
        torch.cuda.synchronize()
        finals[k] = lat.clone()
        log(f"{k}: warmed up")
    for _ in range(args.repeats):
        for k in VARIANTS:
            prepare(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            lat.copy_(x_T)
            e0.record()
            run(samplers[k], VARIANTS[k])
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))

    def identity_level0(steps=4):
        """device events around every launch of `steps` eager steps with PAG on the first level-0 block only"""
        lib.mrisr_prof_reset()
        lib.mrisr_prof_enable(1)
        s = mrisr.Sampler(unet, sched, kind="ddim")
        s.set_range(0, steps)
        lat.copy_(x_T)
        run(s, dict(pag_scale=3.0, pag_applied_layers=("down_blocks.0.attentions.0",)), use_graph=False)
        torch.cuda.synchronize()
        lib.mrisr_prof_enable(0)
        buf = C.create_string_buffer(1 << 20)
        k = lib.mrisr_prof_report(buf, len(buf))
        classes = json.loads(buf.value.decode()) if k > 0 else {}
        lib.mrisr_prof_reset()
        c = classes.get("attn_identity")
        if not c:
            return None
        return {"launches": c["launches"], "us_per_launch": 1e3 * c["ms"] / c["launches"], "bytes_per_launch": c["bytes"] / c["launches"],
                "TB_per_s": c["bytes"] / (c["ms"] * 1e-3) / 1e12}

    out = {"workload": f"SD-1.5-size UNet ({args.dtype}, random init) + rank-4 LoRA, {hw} x {hw} latents, B = {B} slices, {n}-step DDIM, "
                       f"hipGraph; variants timed in alternation after an untimed {args.warmup_steps}-step run of the same variant (plan + "
                       "capture), device events around each whole run",
           "batch": B, "latent": hw, "ddim_steps": n, "repeats": args.repeats, "dtype": args.dtype, "commit": commit_hash(), "variants": {}}
    base = statistics.median(times["plain"])
    for k in VARIANTS:
        ms = statistics.median(times[k])
        out["variants"][k] = {"args": {a: (list(v) if isinstance(v, tuple) else v) for a, v in VARIANTS[k].items()}, "ms_per_run": ms,
                              "ms_per_run_all": times[k], "ms_per_step": ms / n, "slices_per_s": B / (ms * 1e-3),
                              "cost_vs_plain": ms / base, "finite": bool(torch.isfinite(finals[k]).all())}
        log(f"{k}: {ms / n:.2f} ms per step, {ms / base:.3f} x plain")
    out["identity_attention_level0"] = identity_level0()
    log(f"identity attention at level 0: {out['identity_attention_level0']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
