"""GPU: un-merged LoRA adapters of rank 32 .. 128 on the linear targets through the model: the packed layout
(csrc/model.hip::linear), the two-source forward (csrc/runner.h::linear), the backward on the packed banks with ``lora_wgrad_hr``
(csrc/train.hip::linear_bwd) and the refresh of the sB / A^T columns after an optimiser step.

TINY (64 / 128 / 256 / 256), B = 2, 8 x 8 latents, seeded weights, lora_alpha = 2 r.  Reference: tests/lora_ff_ref.py (adapters folded
into float64 weights, autograd through the oracle).  Bounds are those the project applies to rank 4 for the same quantities: 1e-3 (f32
engine: prediction, every gradient tensor, AdamW-updated parameters; tests/test_gpu_unet.py, tests/test_gpu_train.py), 5e-2 (bf16 forward;
tests/test_gpu_unet.py), 6e-2 (bf16 step: prediction, loss, relative L2 of the flat gradient; tests/test_gpu_lora_ff.py), bit equality of graph replay against eager launches
(tests/test_gpu_unet.py), 1e-6 for fit against the hand-driven trainer (tests/test_gpu_fit.py)."""
import ctypes as C_
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_ff_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

B, H, L = 2, 8, 8
ATTN_FF = ref.ATTN + (ref.FF1, ref.FF2)
TOL = {"f32": 1e-3, "bf16": 5e-2}       # forward: tests/test_gpu_unet.py::test_unet_forward_matches_oracle
TOL_GRAD = {"f32": 1e-3, "bf16": 6e-2}  # prediction / loss / flat gradient of the step: tests/test_gpu_train.py, tests/test_gpu_lora_ff.py


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_batch(cfg, seed, b=B, h=H, ctx_len=L):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, 4, h, h), generator=g)
    ctx = torch.randn((b, ctx_len, cfg.cross_attention_dim), generator=g)
    tgt = torch.randn((b, 4, h, h), generator=g)
    t = torch.randint(0, 1000, (b,), generator=g)
    return x, t, ctx, tgt


def build(cfg, up, lora, r, dt, fused=True):
    import mrisr
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype=dt, lora_rank=r, lora_alpha=2.0 * r, lora_fused=fused)
    net.load_state_dict({**up, **lora})
    return net


def prof(fn):
    from mrisr import _lib as L_
    lib = L_.lib()
    lib.mrisr_prof_reset(); lib.mrisr_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.mrisr_prof_enable(0)
    buf = C_.create_string_buffer(1 << 20)
    n = lib.mrisr_prof_report(buf, len(buf))
    names = set(json.loads(buf.value[:n].decode()))
    lib.mrisr_prof_reset()
    return names


@pytest.fixture(scope="module")
def tiny32():
    """TINY with rank-32 adapters on the attention and feed-forward targets, one batch, the float64 step of the reference (shared)."""
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=1811, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_FF), 32, seed=1812)
    batch = make_batch(cfg, 1813)
    x, t, ctx, tgt = batch
    pred, loss, grads = ref.loss_and_grads(cfg, up, lora, 2.0, x, t, ctx, tgt)
    return cfg, up, lora, batch, pred, loss, grads


@pytest.mark.parametrize("r", [32, 48])
def test_forward_fused_matches_oracle_attention_targets(r):
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=1801, perturb_norm=True)
    lora = ou.init_lora_params(up, rank=r, seed=1802)
    for k in lora:  # peft initialises lora_B to zero: make the branch live
        if ".lora_B." in k:
            lora[k] = 0.02 * torch.randn(lora[k].shape, generator=torch.Generator().manual_seed(1803))
    x, t, ctx, _ = make_batch(cfg, 1804)
    with torch.no_grad():
        want = ref.forward(cfg, up, lora, 2.0, x, t, ctx)
        bare = ou.unet_forward({k: v.double() for k, v in up.items()}, cfg, x.double(), t, ctx.double())
    assert rel(bare, want) > 1e-2  # the adapters matter
    for dt in ("f32", "bf16"):
        out = build(cfg, up, lora, r, dt)(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
        print(f"[{dt} r={r}] fused forward vs oracle rel-L2 {rel(out, want):.3e} (<= {TOL[dt]:.0e})")
        assert rel(out, want) < TOL[dt]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_fused_matches_oracle_and_merged_with_ff_targets(tiny32, dt):
    cfg, up, lora, (x, t, ctx, _), want, _, _ = tiny32
    fused = build(cfg, up, lora, 32, dt, True)(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
    merged = build(cfg, up, lora, 32, dt, False)(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
    print(f"[{dt}] fused vs oracle {rel(fused, want):.3e}; fused vs merged on the same engine {rel(fused, merged):.3e}")
    assert rel(fused, want) < TOL[dt]
    assert rel(fused, merged) < TOL[dt]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_real_width_tile_routes_rank_64(dt):
    """320 / 640 channels (the config of tests/test_gpu_ops.py's fp8 test), r = 64: K = 320 + 192 and 640 + 192 through OUT_HEADS, the
    adapted GEGLU projection and ff.net.2 at K = 4C + 64"""
    from oracle import unet as ou
    cfg = ou.UNetConfig(block_out_channels=(320, 640), attn_levels=(True, True), cross_attention_dim=64)
    up = ou.init_unet_params(cfg, seed=1821, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_FF), 64, seed=1822)
    x, t, ctx, _ = make_batch(cfg, 1823, b=1, h=16, ctx_len=77)
    with torch.no_grad():
        want = ref.forward(cfg, up, lora, 2.0, x, t, ctx)
    out = build(cfg, up, lora, 64, dt)(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
    print(f"[{dt}] 320 / 640, r = 64: rel-L2 {rel(out, want):.3e} (<= {TOL[dt]:.0e})")
    assert rel(out, want) < TOL[dt]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gradients_match_autograd(tiny32, dt):
    import mrisr
    cfg, up, lora, (x, t, ctx, tgt), pred_ref, loss_ref, gref = tiny32
    tr = mrisr.LoRATrainer(build(cfg, up, lora, 32, dt))
    assert [k for k, _, _ in tr.layout] == list(lora)
    tr.zero_grad()
    names = prof(lambda: tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda()))
    assert "lora_wgrad_hr" in names and "lora_wgrad" not in names, sorted(names)
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    flat_ref = torch.cat([gref[k].reshape(-1) for k, _, _ in tr.layout])
    print(f"[{dt}] pred {rel(pred, pred_ref):.3e}, loss {float(loss):.6f} vs {loss_ref:.6f}, flat gradient rel-L2 {rel(tr.grad, flat_ref):.3e} (<= {TOL_GRAD[dt]:.0e})")
    assert rel(pred, pred_ref) < TOL_GRAD[dt] and abs(float(loss) - loss_ref) / loss_ref < TOL_GRAD[dt]
    assert rel(tr.grad, flat_ref) < TOL_GRAD[dt]
    if dt == "f32":
        grads = tr.gradients()
        worst = max((rel(grads[k], gref[k]), k) for k in gref)
        print(f"[f32] worst gradient tensor {worst}")
        assert worst[0] < 1e-3, worst


def test_two_optimizer_steps_match_adamw(tiny32):
    """the second step runs on the re-packed sB / A^T columns: a stale column shows here"""
    import mrisr
    cfg, up, lora, (x, t, ctx, tgt), _, _, _ = tiny32
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)
    net = build(cfg, up, lora, 32, "f32")
    tr = mrisr.LoRATrainer(net, **kw)
    lp = ref.leaves(lora)
    opt = torch.optim.AdamW(list(lp.values()), lr=kw["lr"], betas=kw["betas"], weight_decay=kw["weight_decay"], eps=kw["eps"])
    for step in range(2):
        opt.zero_grad()
        with torch.enable_grad():
            loss_ref = torch.nn.functional.mse_loss(ref.forward(cfg, up, lp, 2.0, x, t, ctx), tgt.double())
            loss_ref.backward()
        torch.nn.utils.clip_grad_norm_(list(lp.values()), 1.0)
        opt.step()
        loss = tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda())
        sd = tr.state_dict()
        worst = max((rel(sd[k], lp[k]), k) for k in lp)
        print(f"step {step}: loss {float(loss):.6f} vs {float(loss_ref):.6f}; worst updated tensor {worst}")
        assert abs(float(loss) - float(loss_ref)) / float(loss_ref) < 1e-3
        assert worst[0] < 1e-3, worst
    with torch.no_grad():
        want = ref.forward(cfg, up, {k: v.detach() for k, v in lp.items()}, 2.0, x, t, ctx)
        stale = ref.forward(cfg, up, lora, 2.0, x, t, ctx)
    got = net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
    assert rel(got, want) < 1e-3 and rel(got, stale) > 4 * rel(got, want)


def test_sampler_graph_equals_eager(tiny32):
    import mrisr
    cfg, up, lora, (x, _, ctx, _), _, _, _ = tiny32
    for dt in ("f32", "bf16"):
        net = build(cfg, up, lora, 32, dt)
        finals = {}
        for graph in (True, False):
            sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
            sched.set_timesteps(5)
            lat = x.cuda().clone().contiguous()
            mrisr.Sampler(net, sched, kind="ddim").run(lat, ctx.cuda(), use_graph=graph)
            torch.cuda.synchronize()
            finals[graph] = lat.float().cpu()
        assert bool(torch.isfinite(finals[True]).all()) and torch.equal(finals[True], finals[False]), dt


def test_checkpoint_round_trip_and_rank_mismatch(tiny32, tmp_path):
    import mrisr
    cfg, up, lora, (x, t, ctx, tgt), _, _, _ = tiny32
    net = build(cfg, up, lora, 32, "f32")
    tr = mrisr.LoRATrainer(net, lr=1e-2)
    tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda())
    want = net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
    path = str(tmp_path / "pytorch_lora_weights.safetensors")
    tr.save_checkpoint(path)
    net2 = build(cfg, up, lora, 32, "f32")
    tr2 = mrisr.LoRATrainer(net2, lr=1e-2)
    tr2.load_checkpoint(path)
    got = net2(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
    assert torch.equal(got, want)
    assert not torch.equal(got, build(cfg, up, lora, 32, "f32")(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample)
    # an r = 32 state dict into a model built for rank 4: refused by name, before any parameter is pushed
    net4 = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=8.0, lora_fused=True)
    with pytest.raises(ValueError, match="rank 32"):
        net4.load_state_dict({**up, **lora})
    assert not net4._params and not net4._finalized


def test_fit_equals_the_hand_driven_trainer(tmp_path):
    import mrisr
    from oracle import unet as ou
    from oracle import vae as ov
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=1851, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_FF), 32, seed=1852)
    vp = ov.init_vae_params(ov.TINY_VAE, seed=1853)
    g = torch.Generator().manual_seed(1854)
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    prompts = ["", "an axial T2 slice", "an axial T1 slice"]
    items = []
    for i in range(8):
        hr = (torch.sin(xx / (3 + i % 7)) * torch.cos(yy / (4 + i % 5)) + 0.1 * torch.randn((64, 64), generator=g)).clamp(-1, 1)
        lr = torch.nn.functional.avg_pool2d(hr[None, None], 4).repeat_interleave(4, 2).repeat_interleave(4, 3)[0]
        items.append({"hr": hr[None], "lr": lr, "txt": prompts[1 + i % 2]})
    embeds = {p: torch.randn((L, cfg.cross_attention_dim), generator=g) for p in prompts}

    def models():
        unet = build(cfg, up, lora, 32, "f32")
        vae = mrisr.AutoencoderKL(ov.TINY_VAE, compute_dtype="f32")
        vae.load_state_dict(vp)
        return unet, vae

    c = mrisr.TrainConfig(output_dir=str(tmp_path / "a"), resolution=64, train_batch_size=2, gradient_accumulation_steps=1, max_train_steps=6,
                          learning_rate=1e-3, lr_warmup_steps=1, logging_steps=1, validation_steps=1000, checkpointing_steps=1000,
                          mixed_precision="no", proportion_empty_prompts=0.1, seed=78)
    unet, vae = models()
    res = mrisr.fit(c, unet, vae, items, embeds)
    assert res.step == 6 and bool(np.isfinite(res.losses).all())
    unet_e, _ = models()
    tr = mrisr.LoRATrainer(unet_e, **c.optimizer_kwargs())
    losses = []
    for s in range(c.max_train_steps):
        tr.zero_grad()
        b = res.loop.make_batch(s, 0)
        losses.append(float(tr.forward_backward(b["sample"], b["timesteps"], b["encoder_hidden_states"], b["target"])))
        tr.optimizer_step(world=1, lr=mrisr.cosine_lr(s, c.learning_rate, c.lr_warmup_steps, c.max_train_steps))
    losses = np.asarray(losses)
    print(f"graph vs eager: theta {rel(res.trainer.theta, tr.theta):.3e}, losses {np.abs(res.losses - losses).max():.3e}")
    assert rel(res.trainer.theta, tr.theta) <= 1e-6
    assert np.abs(res.losses - losses).max() <= 1e-6 * np.abs(losses).max()


def test_rank_4_launches_nothing_new():
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=1861, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_FF), 4, seed=1862)
    x, t, ctx, tgt = make_batch(cfg, 1863)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=8.0, lora_fused=True)
    net.load_state_dict({**up, **lora})
    fwd = prof(lambda: net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()))
    tr = mrisr.LoRATrainer(net)
    step = prof(lambda: tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda()))
    assert "lora_wgrad" in step
    for names in (fwd, step):
        assert "lora_wgrad_hr" not in names and not any("_hr" in n for n in names), sorted(names)


def test_rank_16_trains_at_real_width():
    """320 / 640 channels, bf16, r = 16: the dgrad of a K = 320 / 640 projection with a rank above 4 stays off the row-panel kernel (it
    was planned onto it and refused at launch); the step against float64 autograd, bounds of the bf16 step"""
    import mrisr
    from oracle import unet as ou
    cfg = ou.UNetConfig(block_out_channels=(320, 640), attn_levels=(True, True), cross_attention_dim=64)
    up = ou.init_unet_params(cfg, seed=1871, perturb_norm=True)
    lora = ref.init_adapters(up, ref.block_modules(up, ATTN_FF), 16, seed=1872)
    x, t, ctx, tgt = make_batch(cfg, 1873, b=1, h=16, ctx_len=77)
    pred_ref, loss_ref, gref = ref.loss_and_grads(cfg, up, lora, 2.0, x, t, ctx, tgt)
    tr = mrisr.LoRATrainer(build(cfg, up, lora, 16, "bf16"))
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    flat_ref = torch.cat([gref[k].reshape(-1) for k, _, _ in tr.layout])
    print(f"[bf16 r=16, 320 / 640] pred {rel(pred, pred_ref):.3e}, flat gradient rel-L2 {rel(tr.grad, flat_ref):.3e} (<= 6e-2)")
    assert rel(pred, pred_ref) < TOL_GRAD["bf16"] and rel(tr.grad, flat_ref) < TOL_GRAD["bf16"]
