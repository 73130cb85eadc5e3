#!/usr/bin/env python3
"""Optimiser steps per second of ``mrisr.fit`` (two captured graphs per step, no host sync inside a step) next to the hand-driven
eager loop on the SAME batches (``FitLoop.make_batch`` -> ``LoRATrainer.forward_backward`` -> ``optimizer_step``),
in one process: SD-1.5 UNet + r=4 LoRA, SD-1.5 VAE, random weights, ``resolution`` 256 (32 x 32 latents), B = 2 and B = 32.
``--adapter``: the notebook's T2I-Adapter run instead - SD-1.5 UNet frozen (``lora_rank=0``) + full ``Adapter_XL(sk=True, cin=192)``
with EMA, the eager leg ``make_batch`` + ``make_condition(form=0)`` -> ``AdapterTrainer.forward`` -> ``forward_backward(feature_grads=)``
-> ``AdapterTrainer.backward`` -> clip -> AdamW -> EMA.  Not the headline metric (bench.py is) - a line for DESIGN.md.

  python tools/bench_fit.py [--batches 2 32] [--steps 20] [--warmup 3] [--dtype bf16] [--only graph|eager] [--adapter] [--out F]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--only", choices=["graph", "eager"], default=None, help="run one leg only (e.g. under a kernel trace)")
    ap.add_argument("--adapter", action="store_true", help="frozen UNet + trainable Adapter_XL(sk=True) instead of LoRA")
    ap.add_argument("--out", default=None, help="also write the final JSON line to this file")
    args = ap.parse_args()
    import mrisr
    from mrisr import params as P
    dev = torch.device("cuda")
    cfg = mrisr.UNetConfig()
    sd = P.random_state_dict(P.unet_param_shapes(cfg), 20260501, dev)
    rank = 0 if args.adapter else 4
    if rank:
        sd.update(P.random_state_dict(P.lora_param_shapes(cfg, rank), 20260504, dev))
    asd = None
    if args.adapter:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from bench_train import _adapter_shapes
        asd = P.random_state_dict(_adapter_shapes(), 20260506, dev)

    def make_models(tc):
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype=args.dtype, lora_rank=rank, lora_alpha=rank or None, lora_fused=True)
        unet.load_state_dict(sd)
        tr = mrisr.LoRATrainer(unet, **{**tc.optimizer_kwargs()})
        atr = None
        if args.adapter:
            ad = mrisr.Adapter_XL(compute_dtype=args.dtype)
            ad.load_state_dict(asd)
            atr = mrisr.AdapterTrainer(ad, **{**tc.optimizer_kwargs()})
            atr.ema_init()
        return tr, atr
    vcfg = mrisr.VAEConfig()
    vae = mrisr.AutoencoderKL(vcfg, compute_dtype=args.dtype)
    vae.load_state_dict(P.random_state_dict(mrisr.vae_param_shapes(vcfg), 20260505, dev))
    g = torch.Generator().manual_seed(0)
    R = args.resolution
    n_items = max(args.batches)
    items = [{"hr": torch.rand((1, R, R), generator=g) * 2 - 1, "lr": torch.rand((1, R, R), generator=g) * 2 - 1, "txt": "a slice"}
             for _ in range(n_items)]
    embeds = {"": torch.randn((77, cfg.cross_attention_dim), generator=g), "a slice": torch.randn((77, cfg.cross_attention_dim), generator=g)}
    out = {}
    for B in args.batches:
        total = args.warmup + args.steps
        tc = mrisr.TrainConfig(output_dir=tempfile.mkdtemp(prefix="bench_fit_"), resolution=R, train_batch_size=B, max_train_steps=total,
                               learning_rate=1e-4, lr_warmup_steps=2, logging_steps=total, validation_steps=10 ** 9,
                               checkpointing_steps=10 ** 9, mixed_precision="no" if args.dtype == "f32" else "bf16", seed=7)
        row = {}
        if args.only in (None, "graph"):
            tr, atr = make_models(tc)
            loop = mrisr.FitLoop(tc, tr, vae, items, embeds, use_ema=args.adapter, adapter_trainer=atr)
            loop.set_step(0)

            def graph_step():
                loop.micro()
                loop.apply()
            for _ in range(args.warmup):
                graph_step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                graph_step()
            torch.cuda.synchronize()
            row["graph_steps_per_s"] = args.steps / (time.perf_counter() - t0)
            row["graph_captures"] = loop.num_captures
        if args.only in (None, "eager"):
            tr, atr = make_models(tc)
            if args.only == "eager" or "graph_steps_per_s" not in row:
                loop = mrisr.FitLoop(tc, tr, vae, items, embeds, use_ema=args.adapter, adapter_trainer=atr)

            def eager_step(s):
                lr = mrisr.cosine_lr(s, tc.learning_rate, tc.lr_warmup_steps, total)
                b = loop.make_batch(s, 0)
                if atr is None:
                    tr.zero_grad()
                    tr.forward_backward(b["sample"], b["timesteps"], b["encoder_hidden_states"], b["target"])
                    tr.optimizer_step(lr=lr)
                    return
                atr.zero_grad()
                feats = atr.forward(loop.make_condition(s, 0, form=0))
                fg = atr.new_feature_grads()
                tr.forward_backward(b["sample"], b["timesteps"], b["encoder_hidden_states"], b["target"],
                                    down_intrablock_additional_residuals=feats, feature_grads=fg)
                atr.backward(fg)
                atr.optimizer_step(lr=lr, sumsq=atr.sumsq())
                atr.ema_step()
            for s in range(args.warmup):
                eager_step(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.warmup, total):
                eager_step(s)
            torch.cuda.synchronize()
            row["eager_steps_per_s"] = args.steps / (time.perf_counter() - t0)
        if "graph_steps_per_s" in row and "eager_steps_per_s" in row:
            row["speedup"] = row["graph_steps_per_s"] / row["eager_steps_per_s"]
        out[f"B{B}"] = row
        print(json.dumps({"batch": B, **row}), flush=True)
    line = json.dumps({"bench_fit": out, "dtype": args.dtype, "resolution": R, "steps": args.steps,
                       "workload": "frozen UNet + Adapter_XL(sk=True, cin=192), EMA" if args.adapter else "UNet + LoRA r=4"})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
