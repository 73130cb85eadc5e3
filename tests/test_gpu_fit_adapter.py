"""GPU: ``mrisr.fit(adapter=...)`` - the T2I-Adapter trained inside the two captured graphs, with a frozen UNet (the notebook's
``lora_rank: null`` run) or alongside LoRA.  TINY UNet + ADAPTER_TINY + TINY VAE, f32, 64 x 64 pixels: the condition builder
bit for bit, the graph loop against the hand-driven eager loop, loss descent, resume, checkpoints, validation, refusals and a
world-1 RCCL process group."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

PROMPTS = ["", "an axial T2 slice", "an axial T1 slice"]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def setup():
    from oracle import adapter as oa
    from oracle import unet as ou
    from oracle import vae as ov
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=401, perturb_norm=True)
    lp = ou.init_lora_params(up, rank=4, seed=402)
    vp = ov.init_vae_params(ov.TINY_VAE, seed=403)
    ap = oa.init_adapter_params(oa.ADAPTER_TINY, seed=405)
    g = torch.Generator().manual_seed(404)
    y, x = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    items = []
    for i in range(16):
        hr = (torch.sin(x / (3 + i % 7)) * torch.cos(y / (4 + i % 5)) + 0.1 * torch.randn((64, 64), generator=g)).clamp(-1, 1)
        lr = torch.nn.functional.avg_pool2d(hr[None, None], 4).repeat_interleave(4, 2).repeat_interleave(4, 3)[0]
        items.append({"hr": hr[None], "lr": lr, "txt": PROMPTS[1 + i % 2]})
    embeds = {p: torch.randn((16, cfg.cross_attention_dim), generator=g) for p in PROMPTS}
    return cfg, up, lp, vp, ap, items, embeds


def models(setup, lora=False, adapter_dtype="f32"):
    import mrisr
    from oracle import adapter as oa
    from oracle import vae as ov
    cfg, up, lp, vp, ap, _, _ = setup
    if lora:
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4, lora_fused=True)
        unet.load_state_dict({**up, **lp})
    else:
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=0, lora_fused=True)
        unet.load_state_dict(up)
    vae = mrisr.AutoencoderKL(ov.TINY_VAE, compute_dtype="f32")
    vae.load_state_dict(vp)
    ac = oa.ADAPTER_TINY
    ad = mrisr.Adapter_XL(channels=ac.channels, nums_rb=ac.nums_rb, cin=ac.cin, ksize=ac.ksize, compute_dtype=adapter_dtype)
    ad.load_state_dict(ap)
    return unet, vae, ad


def config(tmp, **kw):
    import mrisr
    base = dict(output_dir=str(tmp), resolution=64, train_batch_size=2, gradient_accumulation_steps=1, max_train_steps=10,
                learning_rate=1e-3, lr_warmup_steps=3, logging_steps=5, validation_steps=1000, checkpointing_steps=1000,
                mixed_precision="no", proportion_empty_prompts=0.1, seed=4321)
    base.update(kw)
    return mrisr.TrainConfig(**base)


def test_condition_builder_is_pixel_unshuffle_of_the_drawn_items(setup, tmp_path):
    import mrisr
    from mrisr.fit import FitLoop
    _, _, _, _, _, items, embeds = setup
    unet, vae, ad = models(setup)
    cfg = config(tmp_path, train_batch_size=8, max_train_steps=8, gradient_accumulation_steps=2)
    loop = FitLoop(cfg, mrisr.LoRATrainer(unet), vae, items, embeds, adapter_trainer=mrisr.AdapterTrainer(ad))
    for s, k in ((0, 0), (5, 1), (7, 1)):
        idx = loop.item_indices(s, k)
        img = torch.stack([items[int(i)]["lr"] for i in idx]).cuda().expand(-1, 3, -1, -1)
        c0 = loop.make_condition(s, k, form=0)
        c1 = loop.make_condition(s, k, form=1)
        assert c0.shape == (8, 3, 64, 64) and torch.equal(c0, img)
        assert c1.shape == (8, 8, 8, 192) and c1.dtype == torch.float32
        assert torch.equal(c1, F.pixel_unshuffle(img, 8).permute(0, 2, 3, 1))
    assert not torch.equal(loop.make_condition(5, 1), loop.make_condition(5, 0))


def _eager(setup, res, cfg, lora, use_ema=True):
    """The hand-driven loop on the same batches: make_batch + make_condition(form=0) -> AdapterTrainer.forward ->
    forward_backward(feature_grads=) -> AdapterTrainer.backward, x accum -> joint clip -> AdamW on each bucket -> EMA."""
    import mrisr
    unet, _, ad = models(setup, lora)
    kw = cfg.optimizer_kwargs()
    tr, atr = mrisr.LoRATrainer(unet, **kw), mrisr.AdapterTrainer(ad, **kw)
    if use_ema:
        if lora:
            tr.ema_init()
        atr.ema_init()
    losses, norms = [], []
    for s in range(cfg.max_train_steps):
        tr.zero_grad()
        atr.zero_grad()
        acc = 0.0
        for k in range(cfg.gradient_accumulation_steps):
            b = res.loop.make_batch(s, k)
            feats = atr.forward(res.loop.make_condition(s, k, form=0))
            fg = atr.new_feature_grads()
            acc += float(tr.forward_backward(b["sample"], b["timesteps"], b["encoder_hidden_states"], b["target"],
                                             down_intrablock_additional_residuals=feats, feature_grads=fg))
            atr.backward(fg)
        total = (tr.sumsq().clone() + atr.sumsq()) if lora else atr.sumsq().clone()
        lr = mrisr.cosine_lr(s, cfg.learning_rate, cfg.lr_warmup_steps, cfg.max_train_steps)
        if lora:
            tr.optimizer_step(world=cfg.gradient_accumulation_steps, lr=lr, sumsq=total)
        atr.optimizer_step(world=cfg.gradient_accumulation_steps, lr=lr, sumsq=total)
        if use_ema:
            if lora:
                tr.ema_step()
            atr.ema_step()
        losses.append(acc / cfg.gradient_accumulation_steps)
        norms.append(float(total.sqrt()) / cfg.gradient_accumulation_steps)
    return tr, atr, np.asarray(losses), np.asarray(norms)


@pytest.mark.parametrize("lora", [False, True], ids=["frozen_unet", "lora_and_adapter"])
def test_graph_loop_equals_eager_loop(setup, tmp_path, lora):
    import mrisr
    _, _, _, _, _, items, embeds = setup
    unet, vae, ad = models(setup, lora)
    # With LoRA the UNet's LoRA weight gradients are reduced with atomics, so even two EAGER runs differ at ~1e-7.  Adam divides
    # by sqrt(v) + eps: with eps = 1e-8, elements whose gradient is mostly rounding noise turn that noise into full-size steps,
    # and runs then drift apart by up to 1e-3.  A larger eps keeps the update linear in such gradients, so the comparison
    # measures the loop, not Adam's amplification of reduction order.  The frozen UNet is deterministic: default eps, 1e-6.
    cfg = config(tmp_path, gradient_accumulation_steps=2, **({"adam_epsilon": 1e-3} if lora else {}))
    res = mrisr.fit(cfg, unet, vae, items[:8], embeds, use_ema=True, adapter=ad)
    assert res.step == 10 and res.loop.num_captures == 2
    tr, atr, losses, norms = _eager(setup, res, cfg, lora)
    tol = 1e-5 if lora else 1e-6
    g = res.adapter_trainer
    for a, b in ((g.theta, atr.theta), (g.exp_avg, atr.exp_avg), (g.exp_avg_sq, atr.exp_avg_sq), (g.ema, atr.ema)):
        assert rel(a, b) <= tol, rel(a, b)
    if lora:
        t = res.trainer
        for a, b in ((t.theta, tr.theta), (t.exp_avg, tr.exp_avg), (t.exp_avg_sq, tr.exp_avg_sq), (t.ema, tr.ema)):
            assert rel(a, b) <= tol, rel(a, b)
    else:
        assert res.trainer.num_trainable == 0
    assert np.abs(res.losses - losses).max() <= 1e-6 * np.abs(losses).max()
    assert np.abs(res.grad_norms - norms).max() <= 1e-5 * norms.max()  # the JOINT norm of both buckets
    assert np.array_equal(res.lrs, np.asarray([np.float32(mrisr.cosine_lr(s, 1e-3, 3, 10)) for s in range(10)]))


def test_loss_falls_resume_reproduces_and_checkpoint_loads(setup, tmp_path):
    import mrisr
    from safetensors.torch import load_file
    from oracle import adapter as oa
    _, _, _, _, _, items, embeds = setup
    kw = dict(max_train_steps=30, train_batch_size=4, learning_rate=3e-3, lr_scheduler_name="constant", checkpointing_steps=10,
              logging_steps=10)
    unet, vae, ad = models(setup)
    full = mrisr.fit(config(tmp_path / "a", **kw), unet, vae, items[:8], embeds, adapter=ad)
    assert full.losses[20:30].mean() < full.losses[0:10].mean(), full.losses
    ck = tmp_path / "a" / "checkpoint-20"
    assert (ck / "t2i_adapter.safetensors").is_file() and (ck / "t2i_adapter.safetensors.optim.pt").is_file()
    assert not (ck / "pytorch_lora_weights.safetensors").exists()  # the UNet is frozen: no LoRA file
    unet2, vae2, ad2 = models(setup)
    resumed = mrisr.fit(config(tmp_path / "b", **kw), unet2, vae2, items[:8], embeds, resume_from=str(ck), adapter=ad2)
    for s in (20, 25, 29):
        b1, b2 = full.loop.make_batch(s, 0), resumed.loop.make_batch(s, 0)
        assert all(torch.equal(b1[k], b2[k]) for k in b1)
        assert torch.equal(full.loop.make_condition(s, 0, form=1), resumed.loop.make_condition(s, 0, form=1))
    assert np.array_equal(resumed.losses[:20], full.losses[:20])
    assert np.abs(resumed.losses[20:] - full.losses[20:]).max() <= 1e-6 * np.abs(full.losses[20:]).max()
    assert rel(resumed.adapter_trainer.theta, full.adapter_trainer.theta) <= 1e-6
    # the final checkpoint: the reference module's own keys, equal to theta, and the oracle Adapter_XL reproduces the features
    sd = load_file(str(tmp_path / "a" / "checkpoint-30" / "t2i_adapter.safetensors"))
    views = full.adapter_trainer.state_dict()
    assert set(sd) == {k for k, _, _ in full.adapter_trainer.layout} == set(views)
    assert all(torch.equal(sd[k], views[k].cpu()) for k in views)
    x = full.loop.make_condition(3, 0, form=0)
    want = oa.adapter_forward({k: v.double() for k, v in sd.items()}, oa.ADAPTER_TINY, x.double().cpu())
    got = full.adapter_trainer.adapter(x)
    for a, b in zip(got, want):
        assert rel(a, b) <= 1e-5, rel(a, b)


def test_validation_recaptures_and_leaves_the_run_unchanged(setup, tmp_path):
    import mrisr
    from PIL import Image
    _, _, _, _, _, items, embeds = setup
    unet, vae, ad = models(setup)
    res = mrisr.fit(config(tmp_path / "v", validation_steps=5), unet, vae, items[:8], embeds, val_dataset=items[8:9], adapter=ad)
    assert [os.path.basename(p) for p in res.validation_paths] == ["step-5.png", "step-10.png"]
    assert all(Image.open(p).size == (3 * 64, 64) for p in res.validation_paths)
    assert res.loop.num_captures == 4  # the validation forwards re-planned UNet and adapter: both graphs captured again
    unet2, vae2, ad2 = models(setup)
    plain = mrisr.fit(config(tmp_path / "p"), unet2, vae2, items[:8], embeds, adapter=ad2)
    assert plain.loop.num_captures == 2
    assert rel(res.adapter_trainer.theta, plain.adapter_trainer.theta) <= 1e-6
    assert np.abs(res.losses - plain.losses).max() <= 1e-6 * np.abs(plain.losses).max()


def test_refusals(setup, tmp_path):
    import mrisr
    from oracle import adapter as oa
    _, _, _, _, _, items, embeds = setup
    unet, vae, ad = models(setup)
    with pytest.raises(ValueError, match="nothing to train"):
        mrisr.fit(config(tmp_path / "n"), unet, vae, items[:8], embeds)
    _, _, ad16 = models(setup, adapter_dtype="bf16")
    with pytest.raises(ValueError, match="compute"):
        mrisr.fit(config(tmp_path / "d"), unet, vae, items[:8], embeds, adapter=ad16)
    with pytest.raises(ValueError, match="multiple of 8"):
        mrisr.fit(config(tmp_path / "r", resolution=60), unet, vae, items[:8], embeds, adapter=ad)
    wc = oa.AdapterConfig(channels=(64, 128, 128, 256), nums_rb=1)
    wrong = mrisr.Adapter_XL(channels=wc.channels, nums_rb=1, cin=192, ksize=3, compute_dtype="f32")
    wrong.load_state_dict(oa.init_adapter_params(wc, seed=9))
    with pytest.raises(ValueError, match="intrablock"):
        mrisr.fit(config(tmp_path / "c"), unet, vae, items[:8], embeds, adapter=wrong)
    # checkpoints resume only into a run of the same mix
    kw = dict(max_train_steps=2, checkpointing_steps=2)
    lunet, lvae, _ = models(setup, lora=True)
    mrisr.fit(config(tmp_path / "l", **kw), lunet, lvae, items[:8], embeds)
    mrisr.fit(config(tmp_path / "a", **kw), unet, vae, items[:8], embeds, adapter=ad)
    unet2, vae2, ad2 = models(setup)
    with pytest.raises(ValueError, match="trained lora"):
        mrisr.fit(config(tmp_path / "x", **kw), unet2, vae2, items[:8], embeds, adapter=ad2, resume_from=str(tmp_path / "l" / "checkpoint-2"))
    lunet2, lvae2, _ = models(setup, lora=True)
    with pytest.raises(ValueError, match="trained adapter"):
        mrisr.fit(config(tmp_path / "y", **kw), lunet2, lvae2, items[:8], embeds, resume_from=str(tmp_path / "a" / "checkpoint-2"))
    # nothing above faulted the device: a run still works
    unet3, vae3, ad3 = models(setup)
    ok = mrisr.fit(config(tmp_path / "z", max_train_steps=2), unet3, vae3, items[:8], embeds, adapter=ad3)
    assert np.all(np.isfinite(ok.losses))


def test_world_one_process_group(setup, tmp_path):
    import torch.distributed as dist
    import mrisr
    _, _, _, _, _, items, embeds = setup
    unet, vae, ad = models(setup)
    ref = mrisr.fit(config(tmp_path / "a", max_train_steps=4), unet, vae, items[:8], embeds, adapter=ad)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        unet2, vae2, ad2 = models(setup)
        got = mrisr.fit(config(tmp_path / "b", max_train_steps=4), unet2, vae2, items[:8], embeds, process_group=dist.group.WORLD,
                        adapter=ad2)
    finally:
        dist.destroy_process_group()
    assert rel(got.adapter_trainer.theta, ref.adapter_trainer.theta) <= 1e-6
    assert np.abs(got.losses - ref.losses).max() <= 1e-6 * np.abs(ref.losses).max()
