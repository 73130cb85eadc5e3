"""GPU: LoRA adapters on the GEGLU projection ``ff.net.0.proj`` in the fine-tuning step (csrc/train.hip, csrc/bwd.hip).  The
projection is stored with its (value, gate) rows interleaved in blocks of 16; the trainable ``lora_B`` [8C, r] stays in PyTorch's row
order (value half, then gate half), so the refresh packs it and the dB reduction un-interleaves it in its scatter.

Small two-level UNet (64 / 128 channels: the smallest widths tests/test_gpu_train.py uses; 4C = 256 / 512), batch 2, 8 x 8 latents,
context length 8, rank 4, non-zero B.  Reference: tests/lora_ff_ref.py (adapters folded into float64 weights, autograd through the
oracle).  Tolerances are those of tests/test_gpu_train.py for the same quantities: 1e-3 (f32 engine: prediction, loss, every gradient
tensor, the flat bucket, AdamW-updated parameters), 6e-2 (bf16: prediction, loss, relative L2 of the bucket); those of
tests/test_gpu_fit.py (1e-6) for the graph loop against the eager loop; those of tests/test_gpu_bwd_ops.py for the kernel alone.

C = 48 (4C = 192, not a multiple of the reduce's tile) cannot be built: the GEMMs need K in whole 128-byte tiles and GroupNorm 32
groups, so the channel counts of this library are multiples of 64.  The kernel-alone test covers half = 48."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_ff_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FF1 = ref.FF1
B, H, L, RANK = 2, 8, 8, 4
ALPHA = 8.0  # lora_alpha / r = 2: a scale other than one
ATTN_AND_FF = ("to_q", "to_k", "to_v", "to_out.0", ref.FF1, ref.FF2)  # the common "attention + feed-forward" target set


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def small_cfg(attn_levels=(True, True)):
    from oracle import unet as ou
    return ou.UNetConfig(block_out_channels=(64, 128), attn_levels=attn_levels, cross_attention_dim=64)


def make_batch(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, H, H), generator=g)
    ctx = torch.randn((B, L, cfg.cross_attention_dim), generator=g)
    tgt = torch.randn((B, 4, H, H), generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    return x, t, ctx, tgt


@pytest.fixture(scope="module")
def nine():
    """Adapters on all nine linears of every block, one batch, and the float64 reference of its step (computed once, shared)."""
    from oracle import unet as ou
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=411, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, "all"), RANK, seed=412)
    batch = make_batch(cfg, 413)
    x, t, ctx, tgt = batch
    pred, loss, grads = ref.loss_and_grads(cfg, up, lora, ALPHA / RANK, x, t, ctx, tgt)
    return cfg, up, lora, batch, pred, loss, grads


def trainer(cfg, up, lora, dt, **kw):
    import mrisr
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype=dt, lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True)
    net.load_state_dict({**up, **lora})
    return net, mrisr.LoRATrainer(net, **kw)


def check_ff_halves(grads, gref, tol):
    """lora_B of ff.net.0.proj, each half on its own and element by element (a difference norm, not a norm of each side: rows that
    are merely permuted fail it)."""
    keys = [k for k in gref if k.endswith(FF1 + ".lora_B.default.weight")]
    assert keys
    for k in keys:
        g, r = grads[k].detach().double().cpu(), gref[k]
        half = r.shape[0] // 2
        assert g.shape == r.shape and half % 16 == 0
        for name, sl in (("value", slice(0, half)), ("gate", slice(half, 2 * half))):
            e = rel(g[sl], r[sl])
            print(f"{k} {name} rows: rel-L2 {e:.3e} (<= {tol:.1e})")
            assert float(r[sl].norm()) > 0 and e < tol, (k, name, e)
        # and the halves are not each other's
        assert rel(g[:half], r[half:]) > 0.5 and rel(g[half:], r[:half]) > 0.5, k


@pytest.mark.parametrize("dt,tol", [("f32", 1e-3), ("bf16", 6e-2)])
def test_gradients_match_autograd_all_nine_linears(nine, dt, tol):
    cfg, up, lora, (x, t, ctx, tgt), pred_ref, loss_ref, gref = nine
    _, tr = trainer(cfg, up, lora, dt)
    assert tr.num_trainable == sum(v.numel() for v in lora.values())
    assert [k for k, _, _ in tr.layout] == list(lora)  # block order: ... attn2.to_out.0, ff.net.0.proj, ff.net.2, proj_out
    for k, v in tr.state_dict().items():
        assert torch.equal(v.cpu(), lora[k]), k       # raw row order in the trainable vector
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    print(f"[{dt}] pred rel-L2 {rel(pred, pred_ref):.3e}, loss {float(loss):.6f} vs {loss_ref:.6f}")
    assert rel(pred, pred_ref) < tol
    assert abs(float(loss) - loss_ref) / loss_ref < tol
    grads = tr.gradients()
    flat_ref = torch.cat([gref[k].reshape(-1) for k, _, _ in tr.layout])
    print(f"[{dt}] flat gradient rel-L2 {rel(tr.grad, flat_ref):.3e} (<= {tol:.1e})")
    assert rel(tr.grad, flat_ref) < tol
    if dt == "f32":
        worst = max((rel(grads[k], gref[k]), k) for k in gref)
        print(f"[f32] worst gradient tensor {worst}")
        assert worst[0] < 1e-3, worst
    check_ff_halves(grads, gref, tol)


def test_only_ff1_adapted_with_an_attention_free_level():
    """ff.net.0.proj is the only entry of each block's share of the flat vector; level 1 is a DownBlock2D (no transformer)."""
    from oracle import unet as ou
    cfg = small_cfg(attn_levels=(True, False))
    up = ou.init_unet_params(cfg, seed=421, perturb_norm=True)
    mods = ref.block_modules(up, [FF1])
    assert len(mods) == 2 + 1 + 3  # level-0 down blocks, the mid block, level-0 up blocks
    lora = ref.init_adapters(up, mods, RANK, seed=422)
    x, t, ctx, tgt = make_batch(cfg, 423)
    pred_ref, loss_ref, gref = ref.loss_and_grads(cfg, up, lora, ALPHA / RANK, x, t, ctx, tgt)
    _, tr = trainer(cfg, up, lora, "f32")
    assert [(k, o) for k, o, _ in tr.layout] == list(zip(lora, np.cumsum([0] + [v.numel() for v in lora.values()])[:-1].tolist()))
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    assert rel(pred, pred_ref) < 1e-3 and abs(float(loss) - loss_ref) / loss_ref < 1e-3
    grads = tr.gradients()
    worst = max((rel(grads[k], gref[k]), k) for k in gref)
    print(f"worst gradient tensor {worst}")
    assert worst[0] < 1e-3, worst
    check_ff_halves(grads, gref, 1e-3)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("half", [16, 48])
@pytest.mark.parametrize("r", [4, 8])
def test_wgrad_scatter_kernel_alone(dt, half, r):
    """mrisr_op_lora_wgrad_geglu against float64, in the manner of tests/test_gpu_bwd_ops.py: inputs rounded to the dtype under test,
    float64 reference on them, the kernel adds into a non-zero prior; relative L2 <= 1e-3 (f32 output) and, element-wise with no
    element excluded, |got - ref| <= floor with floor = 8 x the largest deviation of the same formula in plain torch float32 on the
    CPU from the float64 reference (f32 arithmetic noise; measured here, on these inputs, without the kernel).  M = 70: one block of
    rows with a ragged tail; M = 1100: more than one row slab for every geometry (bf16 half = 16: 1024 rows per block)."""
    from mrisr import ops
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}[dt]
    perm = ops.geglu_packed_rows(half)
    for M, scale in ((70, 1.0), (1100, 0.375)):
        g = torch.Generator().manual_seed(431 + M + half + r)
        dpre_raw = torch.randn((M, 2 * half), generator=g).to(tdt)      # columns in lora_B's row order: value | gate
        z = torch.randn((M, r), generator=g)
        prior = torch.randn((2 * half, r), generator=g)
        packed = torch.empty_like(dpre_raw)
        packed[:, perm] = dpre_raw                                       # what geglu_bwd hands over
        want = prior.double() + scale * dpre_raw.double().t() @ z.double()
        floor = 8 * float((prior + scale * dpre_raw.float().t() @ z - want).abs().max())
        out = prior.cuda().clone()
        ops.lora_wgrad_geglu(packed.cuda().contiguous(), z.cuda(), out, scale)
        got = out.double().cpu()
        l2, worst = rel(got, want), float((got - want).abs().max())
        print(f"lora_wgrad_geglu[{dt} M={M} half={half} r={r}]: rel-L2 {l2:.3e} (<= 1e-3), max |d| {worst:.3e} (<= floor {floor:.3e})")
        assert l2 <= 1e-3 and worst <= floor
        for name, sl in (("value", slice(0, half)), ("gate", slice(half, 2 * half))):
            assert rel(got[sl], want[sl]) <= 1e-3, name


def test_wgrad_scatter_kernel_refuses_bad_arguments():
    import mrisr
    from mrisr import ops
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    for bad in (lambda: ops.lora_wgrad_geglu(f32(8, 48), f32(8, 4), f32(48, 4)),       # half = 24: not whole 16-blocks
                lambda: ops.lora_wgrad_geglu(f32(8, 64), f32(8, 6), f32(64, 6)),       # rank 6
                lambda: ops.lora_wgrad_geglu(f32(8, 64), f32(8, 4), f32(64, 4), ldp=32)):  # pitch below the row
        with pytest.raises(mrisr.MrisrError):
            bad()


def test_optimizer_step_and_refresh_in_packed_order(nine):
    """One LoRATrainer.step against float64 AdamW (+ clip_grad_norm_ 1.0) on the autograd gradients of the shared reference; the UNet
    forward afterwards runs on the refreshed adapters - loraB of ff.net.0.proj re-packed into the interleaved row order from the
    raw-order trainable tensor."""
    cfg, up, lora, (x, t, ctx, tgt), _, loss_val, gref = nine
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)
    net, tr = trainer(cfg, up, lora, "f32", **kw)
    lp = ref.leaves(lora)
    opt = torch.optim.AdamW(list(lp.values()), lr=kw["lr"], betas=kw["betas"], weight_decay=kw["weight_decay"], eps=kw["eps"])
    for k, v in lp.items():
        v.grad = gref[k].clone()
    loss_ref = torch.tensor(loss_val)
    norm_ref = float(torch.nn.utils.clip_grad_norm_(list(lp.values()), 1.0))
    opt.step()
    loss = tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda())
    assert abs(float(loss) - float(loss_ref.detach())) / float(loss_ref.detach()) < 1e-3
    assert abs(tr.grad_norm() - norm_ref) / norm_ref < 1e-3
    sd = tr.state_dict()
    worst = max((rel(sd[k], lp[k]), k) for k in lp)
    print(f"gradient norm {norm_ref:.4f}; worst updated tensor {worst}")
    assert worst[0] < 1e-3, worst
    for k in lp:
        if FF1 in k:
            assert rel(sd[k], lora[k]) > 1e-3, k  # ... and they did move
    x2, t2, ctx2, _ = make_batch(cfg, 441)
    with torch.no_grad():
        want = ref.forward(cfg, up, {k: v.detach() for k, v in lp.items()}, ALPHA / RANK, x2, t2, ctx2)
        stale = ref.forward(cfg, up, lora, ALPHA / RANK, x2, t2, ctx2)
    got = net(x2.cuda(), t2.cuda(), encoder_hidden_states=ctx2.cuda()).sample
    print(f"post-step forward rel-L2 {rel(got, want):.3e}; against the adapters before the step {rel(got, stale):.3e}")
    assert rel(got, want) < 1e-3
    assert rel(got, stale) > 4 * rel(got, want)


def test_inference_forward_applies_the_ff1_adapter(nine):
    """UNet2DConditionModel.forward with un-merged adapters on ff.net.0.proj, without a trainer: both engines against the oracle
    (bounds of tests/test_gpu_unet.py / test_gpu_train.py for the forward: 1e-3 f32, 6e-2 bf16)."""
    import mrisr
    cfg, up, lora, (x, t, ctx, _), pred_ref, _, _ = nine
    from oracle import unet as ou
    with torch.no_grad():
        bare = ou.unet_forward({k: v.double() for k, v in up.items()}, cfg, x.double(), t, ctx.double())
    for dt, tol in (("f32", 1e-3), ("bf16", 6e-2)):
        net = mrisr.UNet2DConditionModel(cfg, compute_dtype=dt, lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True)
        net.load_state_dict({**up, **lora})
        out = net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
        print(f"[{dt}] forward rel-L2 {rel(out, pred_ref):.3e}; the adapters change the output by {rel(bare, pred_ref):.3e}")
        assert rel(out, pred_ref) < tol


def test_fp8_train_refuses_an_adapted_ff1(nine):
    import mrisr
    cfg, up, lora, *_ = nine
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True, fp8=True,
                                     fp8_train=True)
    net.load_state_dict({**up, **lora})
    with pytest.raises(mrisr.MrisrError, match="fp8_train"):
        mrisr.LoRATrainer(net)


# ---- mrisr.fit ----
PROMPTS = ["", "an axial T2 slice", "an axial T1 slice"]


def test_fit_trains_ff_adapters_and_resumes(tmp_path):
    """Two optimiser steps of two micro-batches inside the captured graphs M and O equal the eager loop on the same batches
    (make_batch + forward_backward + optimizer_step), to 1e-6 as tests/test_gpu_fit.py asks of the same comparison; the checkpoint
    of step 1 carries the ff.net.0.proj tensors and resumes to the same final state."""
    import mrisr
    from oracle import unet as ou
    from oracle import vae as ov
    from safetensors.torch import load_file
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=451, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_AND_FF), RANK, seed=452)
    vp = ov.init_vae_params(ov.TINY_VAE, seed=453)
    g = torch.Generator().manual_seed(454)
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    items = []
    for i in range(8):
        hr = (torch.sin(xx / (3 + i % 7)) * torch.cos(yy / (4 + i % 5)) + 0.1 * torch.randn((64, 64), generator=g)).clamp(-1, 1)
        lr = torch.nn.functional.avg_pool2d(hr[None, None], 4).repeat_interleave(4, 2).repeat_interleave(4, 3)[0]
        items.append({"hr": hr[None], "lr": lr, "txt": PROMPTS[1 + i % 2]})
    embeds = {p: torch.randn((L, cfg.cross_attention_dim), generator=g) for p in PROMPTS}

    def models():
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True)
        unet.load_state_dict({**up, **lora})
        vae = mrisr.AutoencoderKL(ov.TINY_VAE, compute_dtype="f32")
        vae.load_state_dict(vp)
        return unet, vae

    def config(out):
        return mrisr.TrainConfig(output_dir=str(out), resolution=64, train_batch_size=2, gradient_accumulation_steps=2, max_train_steps=2,
                                 learning_rate=1e-3, lr_warmup_steps=1, logging_steps=1, validation_steps=1000, checkpointing_steps=1,
                                 mixed_precision="no", proportion_empty_prompts=0.1, seed=77)

    unet, vae = models()
    c = config(tmp_path / "a")
    res = mrisr.fit(c, unet, vae, items, embeds)
    assert res.step == 2 and res.loop.num_captures == 2
    ff_keys = [k for k, _, _ in res.trainer.layout if FF1 in k]
    assert len(ff_keys) == 2 * len(ref.block_modules(up, [FF1])) == 2 * 11

    unet_e, _ = models()
    tr = mrisr.LoRATrainer(unet_e, **c.optimizer_kwargs())
    losses = []
    for s in range(c.max_train_steps):
        tr.zero_grad()
        acc = 0.0
        for k in range(c.gradient_accumulation_steps):
            b = res.loop.make_batch(s, k)
            acc += float(tr.forward_backward(b["sample"], b["timesteps"], b["encoder_hidden_states"], b["target"]))
        tr.optimizer_step(world=c.gradient_accumulation_steps, lr=mrisr.cosine_lr(s, c.learning_rate, c.lr_warmup_steps, c.max_train_steps))
        losses.append(acc / c.gradient_accumulation_steps)
    losses = np.asarray(losses)
    print(f"graph vs eager: theta {rel(res.trainer.theta, tr.theta):.3e}, losses {np.abs(res.losses - losses).max():.3e}")
    assert rel(res.trainer.theta, tr.theta) <= 1e-6
    assert np.abs(res.losses - losses).max() <= 1e-6 * np.abs(losses).max()
    sd0, sd1 = {k: v for k, v in lora.items()}, res.trainer.state_dict()
    assert all(not torch.equal(sd1[k].cpu(), sd0[k]) for k in ff_keys)  # step 2 runs at a non-zero learning rate

    # the checkpoints carry the new tensors under peft's on-disk keys ...
    ck1, ck2 = (os.path.join(str(tmp_path / "a"), f"checkpoint-{n}") for n in (1, 2))
    disk = mrisr.train.lora_keys_from_disk(load_file(os.path.join(ck2, "pytorch_lora_weights.safetensors")))
    assert set(disk) == set(sd1) and all(torch.equal(disk[k], sd1[k].cpu()) for k in sd1)
    # ... and the run resumed from step 1 ends where the uninterrupted one did
    unet_r, vae_r = models()
    resumed = mrisr.fit(config(tmp_path / "b"), unet_r, vae_r, items, embeds, resume_from=ck1)
    assert resumed.step == 2
    assert rel(resumed.trainer.theta, res.trainer.theta) <= 1e-6
    assert abs(float(resumed.losses[1]) - float(res.losses[1])) <= 1e-6 * abs(float(res.losses[1]))


def test_joint_steps_with_an_adapted_ff1():
    """joint_step and joint_step_overlapped (T2I-Adapter + LoRA) on a UNet with ff adapters: both run and agree with each other, as
    tests/test_gpu_train.py asks of the two on attention adapters (same loss, parameters to 1e-6)."""
    import mrisr
    from oracle import adapter as oa
    from oracle import unet as ou
    cfg = ou.TINY  # the T2I-Adapter has four levels: the four-level UNet of tests/test_gpu_train.py
    up = ou.init_unet_params(cfg, seed=461, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_AND_FF), RANK, seed=462)
    acfg = oa.AdapterConfig(channels=(64, 128, 256, 256), nums_rb=2, cin=192, ksize=3)
    ap = oa.init_adapter_params(acfg, seed=463)
    x, t, ctx, tgt = make_batch(cfg, 464)
    cond = torch.randn((B, 3, 8 * H, 8 * H), generator=torch.Generator().manual_seed(465))

    def run(step_fn):
        _, ltr = trainer(cfg, up, lora, "f32", lr=1e-3, max_grad_norm=1.0)
        ad = mrisr.Adapter_XL(channels=acfg.channels, nums_rb=acfg.nums_rb, cin=acfg.cin, ksize=acfg.ksize, compute_dtype="f32")
        ad.load_state_dict(ap)
        atr = mrisr.AdapterTrainer(ad, lr=1e-3, max_grad_norm=1.0)
        loss = float(step_fn(ltr, atr, x.cuda(), t.cuda(), ctx.cuda(), (50.0 * tgt).cuda(), cond.cuda()))
        return ltr, atr, loss

    l0, a0, loss0 = run(mrisr.joint_step)
    l1, a1, loss1 = run(mrisr.joint_step_overlapped)
    assert loss1 == loss0 and rel(l1.theta, l0.theta) < 1e-6 and rel(a1.theta, a0.theta) < 1e-6
    moved = [k for k, v in l0.state_dict().items() if FF1 in k and not torch.equal(v.cpu(), lora[k])]
    assert len(moved) == 2 * len(ref.block_modules(up, [FF1])) == 2 * 16


# ---- nothing moved for existing users ----
def test_layout_without_ff1_adapters_is_unchanged():
    """Adapters on the eight linears the trainer already took: keys, shapes, order and count of the flat vector, computed here from the
    config as r (in + out) per target in the existing order."""
    from oracle import unet as ou
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=471, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, "existing"), RANK, seed=472)
    _, tr = trainer(cfg, up, lora, "f32")
    D = cfg.cross_attention_dim
    want, total = [], 0
    blocks = ([(f"down_blocks.{i}.attentions.{j}", c) for i, c in enumerate(cfg.block_out_channels) for j in range(cfg.layers_per_block)]
              + [("mid_block.attentions.0", cfg.block_out_channels[-1])]
              + [(f"up_blocks.{i}.attentions.{j}", c) for i, c in enumerate(reversed(cfg.block_out_channels))
                 for j in range(cfg.layers_per_block + 1)])
    for b, c in blocks:
        t = b + ".transformer_blocks.0."
        targets = [(b + ".proj_in", c, c), (t + "attn1.to_q", c, c), (t + "attn1.to_k", c, c), (t + "attn1.to_v", c, c),
                   (t + "attn1.to_out.0", c, c), (t + "attn2.to_q", c, c), (t + "attn2.to_k", c, D), (t + "attn2.to_v", c, D),
                   (t + "attn2.to_out.0", c, c), (t + "ff.net.2", c, 4 * c), (b + ".proj_out", c, c)]
        for m, n_out, n_in in targets:
            want += [(m + ".lora_A.default.weight", (RANK, n_in)), (m + ".lora_B.default.weight", (n_out, RANK))]
            total += RANK * (n_in + n_out)
    assert [(k, tuple(v.shape)) for k, v in tr.state_dict().items()] == want
    assert tr.num_trainable == total
    offs = np.cumsum([0] + [r * c for _, (r, c) in want])[:-1].tolist()
    assert [o for _, o, _ in tr.layout] == offs
