"""GPU: LoRA adapters on the resnet 3x3 convs (peft ``lora.Conv2d``): the two kernels of csrc/lora_conv.hip alone, the conv GEMM's LoRA
epilogue with ``conv = 1``, and the adapters through the trainer, the inference forward, the sampler graph and ``mrisr.fit``.

References are float64 (tests/lora_conv_ref.py: adapters folded into the conv weights, autograd through the oracle).  Tolerances are the
project's own for the same quantities: kernels alone tests/test_gpu_bwd_ops.py ``TOL`` (relative L2 1e-3 for f32 outputs, 1.2e-2 for bf16
outputs); model level 1e-3 for the f32 engine (prediction, loss, every gradient tensor, the bucket) and 6e-2 for bf16 (prediction, loss,
bucket) as tests/test_gpu_train.py / test_gpu_lora_ff.py; graph loop against eager loop 1e-6 as tests/test_gpu_fit.py.

Model: the two-level UNet of tests/test_gpu_lora_ff.py (64 / 128 channels), batch 2, 8 x 8 latents, context length 8, rank 4, alpha 8."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_conv_ref as ref  # noqa: E402
import lora_ff_ref as ffref  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-3, "bf16": 1.2e-2}   # tests/test_gpu_bwd_ops.py
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
B, H, L, RANK = 2, 8, 8, 4
ALPHA = 8.0
SCALE = ALPHA / RANK
ATTN = ("to_q", "to_k", "to_v", "to_out.0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels alone
# ---------------------------------------------------------------------------------------------------------------------------------
DOWN_SHAPES = [(1, 4, 4, 64, 4),      # M = 16: one wave group, every pixel on a border
               (2, 5, 12, 64, 4),     # M = 120: not a multiple of 16, groups straddle rows and the two images
               (3, 3, 7, 64, 4),      # W < 16 and odd
               (2, 8, 8, 128, 8),
               (1, 16, 16, 192, 16),  # R = 16
               (1, 32, 32, 320, 4),   # the level-0 geometry at B = 1
               (2, 4, 4, 1280, 4)]    # a deep level: K split over the waves of a workgroup and over workgroups


def _down_case(shape, dt, seed):
    Bn, Hn, Wn, cin, r = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((Bn, Hn, Wn, cin), generator=g).to(TDT[dt])
    A = ((torch.rand((r, cin, 3, 3), generator=g) * 2 - 1) / (9 * cin) ** 0.5).to(TDT[dt])   # what the packer stores
    want = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), A.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, r)
    return x, A, want


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", DOWN_SHAPES)
def test_conv_lora_down_alone(shape, dt):
    """z = conv3x3(x, A) against F.conv2d on the rounded inputs in float64; z is f32 for both dtypes: relative L2 <= 1e-3.  Two launches
    give the same bits (fixed-order reductions, no float atomics)."""
    from mrisr import ops
    x, A, want = _down_case(shape, dt, 600 + sum(shape))
    xc = x.cuda()
    z1 = ops.conv_lora_down(xc, A.float().cuda())
    z2 = ops.conv_lora_down(xc, A.float().cuda())
    e = rel(z1, want)
    print(f"conv_lora_down[{dt} {shape}]: rel-L2 {e:.3e} (<= {TOL['f32']:.1e})")
    assert z1.dtype == torch.float32 and z1.shape == want.shape
    assert e <= TOL["f32"]
    assert torch.equal(z1, z2)


@pytest.mark.parametrize("shape", [(2, 5, 12, 64, 4), (2, 4, 4, 1280, 4)])
def test_conv_lora_down_every_route(shape):
    """bf16: the pixel-parallel form, the four-wave K split and the K split over 2 / 8 workgroups all compute the same z (to f32 summation
    order) - the planned route of the deep shape is one of the split ones, exercised above."""
    from mrisr import ops
    x, A, want = _down_case(shape, "bf16", 650 + sum(shape))
    for route in (101, 401, 402, 408):
        z = ops.conv_lora_down(x.cuda(), A.float().cuda(), route=route)
        e = rel(z, want)
        print(f"conv_lora_down[bf16 {shape} route {route}]: rel-L2 {e:.3e}")
        assert e <= TOL["f32"], route
        assert torch.equal(z, ops.conv_lora_down(x.cuda(), A.float().cuda(), route=route)), route


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 4, 4, 64, 4), (2, 5, 12, 64, 4), (2, 8, 8, 320, 8), (1, 8, 8, 448, 16), (1, 4, 4, 2560, 4)])
def test_conv_lora_dgrad_alone(shape, dt):
    """dx against the autograd gradient of sum(conv2d(x, A, padding=1) * dz) with respect to x, as a first write and accumulated onto a
    random tensor; the output has the compute dtype: relative L2 <= TOL[dt] (bf16: dz is rounded to bf16 on entry, as documented)."""
    from mrisr import ops
    Bn, Hn, Wn, cin, r = shape
    g = torch.Generator().manual_seed(700 + sum(shape))
    A = ((torch.rand((r, cin, 3, 3), generator=g) * 2 - 1) / (9 * cin) ** 0.5).to(TDT[dt])
    # dz scaled so that dx has about the prior's size: an element of dx sums <= 9 r products of dz with A ~ U(+-1/sqrt(9 cin)), variance
    # 1 / (27 cin) each, so std(dx) = std(dz) sqrt(r / (3 cin)) in the interior and >= 2/3 of it on a border (>= 4 of 9 taps)
    dz = torch.randn((Bn * Hn * Wn, r), generator=g) * (3 * cin / r) ** 0.5
    prior = torch.randn((Bn, Hn, Wn, cin), generator=g).to(TDT[dt])
    xg = torch.zeros((Bn, cin, Hn, Wn), dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        y = torch.nn.functional.conv2d(xg, A.double(), padding=1)
        (y * dz.double().reshape(Bn, Hn, Wn, r).permute(0, 3, 1, 2)).sum().backward()
    want = xg.grad.permute(0, 2, 3, 1)
    got = ops.conv_lora_dgrad(dz.cuda(), A.float().cuda(), Bn, Hn, Wn, dtype=TDT[dt])
    e0 = rel(got, want)
    acc = prior.cuda().clone()
    ops.conv_lora_dgrad(dz.cuda(), A.float().cuda(), Bn, Hn, Wn, dx=acc, acc=True)
    e1 = rel(acc, want + prior.double())
    print(f"conv_lora_dgrad[{dt} {shape}]: first write rel-L2 {e0:.3e}, accumulate {e1:.3e} (<= {TOL[dt]:.1e})")
    assert got.dtype == TDT[dt] and tuple(got.shape) == (Bn, Hn, Wn, cin)
    assert e0 <= TOL[dt] and e1 <= TOL[dt]
    assert rel(acc, prior) > 0.3  # ... and it did add something (std(dx) / std(prior) >= 2/3 by the scaling above)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 8, 8, 64, 128, 1), (2, 8, 8, 64, 128, 2), (1, 16, 16, 64, 64, 0)],
                         ids=["unsplit", "splitk2", "planned-16x16"])
def test_conv3x3_with_lora_epilogue_alone(case, dt):
    """GemmArgs::lora_z with conv = 1: conv + bias + time-embedding row + s B conv3x3(x, A) + residual against F.conv2d with W_eff (+ the
    same row vector and residual), float64 on the rounded inputs.  Un-split, forced split-K 2 (the reduce kernel's epilogue), and whatever
    the planner selects for the 16 x 16 image."""
    from mrisr import ops
    Bn, Hn, Wn, cin, cout, splitk = case
    g = torch.Generator().manual_seed(800 + sum(case))
    t = TDT[dt]
    x = torch.randn((Bn, cin, Hn, Wn), generator=g).to(t)
    w = ((torch.rand((cout, cin, 3, 3), generator=g) * 2 - 1) / (9 * cin) ** 0.5).to(t)
    bias = torch.randn((cout,), generator=g)
    A = ((torch.rand((RANK, cin, 3, 3), generator=g) * 2 - 1) / (9 * cin) ** 0.5).to(t)
    Bm = torch.randn((cout, RANK, 1, 1), generator=g) * 0.5   # large enough that a missing LoRA term fails the bound
    rowvec = torch.randn((Bn, cout), generator=g)
    resid = torch.randn((Bn, cout, Hn, Wn), generator=g).to(t)
    xd = x.double()
    want = ref.two_conv(xd, w.double(), bias.double(), A.double(), Bm.double(), SCALE) + rowvec.double()[:, :, None, None] + resid.double()
    bare = want - SCALE * torch.nn.functional.conv2d(torch.nn.functional.conv2d(xd, A.double(), padding=1), Bm.double())
    got = ops.conv3x3_lora(x.cuda(), w.float().cuda(), bias.cuda(), A.float().cuda(), Bm.cuda(), SCALE, rowvec=rowvec.cuda(), resid=resid.cuda(),
                           splitk=splitk)
    e = rel(got, want)
    print(f"conv3x3_lora[{dt} {case}]: rel-L2 {e:.3e} (<= {TOL[dt]:.1e}); without the adapter {rel(bare, want):.3e}")
    assert e <= TOL[dt]
    assert rel(bare, want) > 4 * TOL[dt]


# ---------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------
def small_cfg(attn_levels=(True, True)):
    from oracle import unet as ou
    return ou.UNetConfig(block_out_channels=(64, 128), attn_levels=attn_levels, cross_attention_dim=64)


def make_batch(cfg, seed, scalar_t=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, H, H), generator=g)
    ctx = torch.randn((B, L, cfg.cross_attention_dim), generator=g)
    tgt = torch.randn((B, 4, H, H), generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    return x, (t[0] if scalar_t else t), ctx, tgt


def trainer(cfg, up, lora, dt, **kw):
    import mrisr
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype=dt, lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True)
    net.load_state_dict({**up, **lora})
    return net, mrisr.LoRATrainer(net, **kw)


@pytest.fixture(scope="module")
def both():
    """Adapters on the attention projections and on every conv1 / conv2, one batch, and the float64 reference of its step (shared)."""
    from oracle import unet as ou
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=511, perturb_norm=True)
    lin = ffref.init_adapters(up, ffref.block_modules(up, ATTN), RANK, seed=512)
    conv = ref.init_adapters(up, ref.resnet_modules(up), RANK, seed=513)
    lora = {**lin, **conv}
    batch = make_batch(cfg, 514)
    x, t, ctx, tgt = batch
    pred, loss, grads = ref.loss_and_grads(cfg, up, lora, SCALE, x, t, ctx, tgt)
    return cfg, up, lin, conv, lora, batch, pred, loss, grads


@pytest.mark.parametrize("dt,tol", [("f32", 1e-3), ("bf16", 6e-2)])
def test_gradients_match_autograd_attention_and_conv_adapters(both, dt, tol):
    cfg, up, lin, conv, lora, (x, t, ctx, tgt), pred_ref, loss_ref, gref = both
    _, tr = trainer(cfg, up, lora, dt)
    assert tr.num_trainable == sum(v.numel() for v in lora.values())
    assert [k for k, _, _ in tr.layout] == list(lin) + list(conv)   # the linear keys first, in today's order; then the resnet walk
    assert len(conv) == 2 * 2 * (4 + 2 + 6)
    offs = np.cumsum([0] + [v.numel() for v in lora.values()])[:-1].tolist()
    assert [o for _, o, _ in tr.layout] == offs
    for k, v in tr.state_dict().items():
        assert v.shape == lora[k].shape and torch.equal(v.cpu(), lora[k]), k   # the loaded tensors, 4-D for the convs, bit for bit
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    flat_ref = torch.cat([gref[k].reshape(-1) for k, _, _ in tr.layout])
    print(f"[{dt}] pred rel-L2 {rel(pred, pred_ref):.3e}, loss {float(loss):.6f} vs {loss_ref:.6f}, bucket rel-L2 {rel(tr.grad, flat_ref):.3e} (<= {tol:.1e})")
    assert rel(pred, pred_ref) < tol
    assert abs(float(loss) - loss_ref) / loss_ref < tol
    assert rel(tr.grad, flat_ref) < tol
    grads = tr.gradients()
    conv_ref = torch.cat([gref[k].reshape(-1) for k in conv])
    conv_got = torch.cat([grads[k].reshape(-1) for k in conv])
    print(f"[{dt}] conv adapters' share of the bucket: rel-L2 {rel(conv_got, conv_ref):.3e}")
    assert rel(conv_got, conv_ref) < tol
    if dt == "f32":
        worst = max((rel(grads[k], gref[k]), k) for k in gref)
        print(f"[f32] worst gradient tensor {worst}")
        assert all(grads[k].shape == gref[k].shape for k in gref)
        assert worst[0] < 1e-3, worst


def test_conv_adapters_only_with_an_attention_free_level():
    """Only conv adapters; level 1 is a DownBlock2D / UpBlock2D (resnets with concat inputs, no transformer); scalar timestep.  The first
    resnet after conv_in has no live input: its backward computes weight gradients only - and they are not zero."""
    from oracle import unet as ou
    cfg = small_cfg(attn_levels=(True, False))
    up = ou.init_unet_params(cfg, seed=521, perturb_norm=True)
    lora = ref.init_adapters(up, ref.resnet_modules(up), RANK, seed=522)
    x, t, ctx, tgt = make_batch(cfg, 523, scalar_t=True)
    pred_ref, loss_ref, gref = ref.loss_and_grads(cfg, up, lora, SCALE, x, t, ctx, tgt)
    _, tr = trainer(cfg, up, lora, "f32")
    assert [k for k, _, _ in tr.layout] == list(lora)
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    assert rel(pred, pred_ref) < 1e-3 and abs(float(loss) - loss_ref) / loss_ref < 1e-3
    grads = tr.gradients()
    worst = max((rel(grads[k], gref[k]), k) for k in gref)
    print(f"worst gradient tensor {worst}")
    assert worst[0] < 1e-3, worst
    first = [k for k in lora if k.startswith("down_blocks.0.resnets.0.")]
    assert len(first) == 4 and all(float(grads[k].abs().max()) > 0 and float(gref[k].abs().max()) > 0 for k in first)


def test_a_subset_conv2_of_the_mid_block():
    from oracle import unet as ou
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=531, perturb_norm=True)
    mods = ref.resnet_modules(up, lambda m: m.startswith("mid_block.") and m.endswith("conv2"))
    assert mods == ["mid_block.resnets.0.conv2", "mid_block.resnets.1.conv2"]
    lora = ref.init_adapters(up, mods, RANK, seed=532)
    x, t, ctx, tgt = make_batch(cfg, 533)
    pred_ref, loss_ref, gref = ref.loss_and_grads(cfg, up, lora, SCALE, x, t, ctx, tgt)
    _, tr = trainer(cfg, up, lora, "f32")
    assert [(k, o, s) for k, o, s in tr.layout] == [(k, o, tuple(v.shape)) for (k, v), o in
                                                    zip(lora.items(), np.cumsum([0] + [v.numel() for v in lora.values()])[:-1].tolist())]
    assert tr.num_trainable == sum(v.numel() for v in lora.values()) == 2 * RANK * (9 * 128 + 128)
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    assert rel(pred, pred_ref) < 1e-3 and abs(float(loss) - loss_ref) / loss_ref < 1e-3
    grads = tr.gradients()
    worst = max((rel(grads[k], gref[k]), k) for k in gref)
    print(f"worst gradient tensor {worst}")
    assert worst[0] < 1e-3, worst


def test_optimizer_step_then_the_refreshed_forward(both):
    """One clip + AdamW step against torch.optim.AdamW on the reference's float64 gradients, then the next prediction on the refreshed
    views (f32, 1e-3)."""
    cfg, up, lin, conv, lora, (x, t, ctx, tgt), _, loss_val, gref = both
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)
    net, tr = trainer(cfg, up, lora, "f32", **kw)
    lp = ref.leaves(lora)
    opt = torch.optim.AdamW(list(lp.values()), lr=kw["lr"], betas=kw["betas"], weight_decay=kw["weight_decay"], eps=kw["eps"])
    for k, v in lp.items():
        v.grad = gref[k].clone()
    norm_ref = float(torch.nn.utils.clip_grad_norm_(list(lp.values()), 1.0))
    opt.step()
    loss = tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda())
    assert abs(float(loss) - loss_val) / loss_val < 1e-3
    assert abs(tr.grad_norm() - norm_ref) / norm_ref < 1e-3
    sd = tr.state_dict()
    worst = max((rel(sd[k], lp[k]), k) for k in lp)
    print(f"gradient norm {norm_ref:.4f}; worst updated tensor {worst}")
    assert worst[0] < 1e-3, worst
    assert all(rel(sd[k], lora[k]) > 1e-3 for k in conv)   # ... and the conv adapters did move
    x2, t2, ctx2, _ = make_batch(cfg, 541)
    with torch.no_grad():
        want = ref.forward(cfg, up, {k: v.detach() for k, v in lp.items()}, SCALE, x2, t2, ctx2)
        stale = ref.forward(cfg, up, lora, SCALE, x2, t2, ctx2)
    got = net(x2.cuda(), t2.cuda(), encoder_hidden_states=ctx2.cuda()).sample
    print(f"post-step forward rel-L2 {rel(got, want):.3e}; against the adapters before the step {rel(got, stale):.3e}")
    assert rel(got, want) < 1e-3
    assert rel(got, stale) > 4 * rel(got, want)


def test_inference_fused_merged_and_sampler_graph(both):
    import mrisr
    from oracle import unet as ou
    cfg, up, lin, conv, lora, (x, t, ctx, _), pred_ref, _, _ = both
    with torch.no_grad():
        bare = ffref.forward(cfg, up, lin, SCALE, x, t, ctx)   # the same model without the conv adapters
    print(f"the conv adapters change the output by {rel(bare, pred_ref):.3e}")
    for dt, tol in (("f32", 1e-3), ("bf16", 6e-2)):
        outs = {}
        for fused in (True, False):
            net = mrisr.UNet2DConditionModel(cfg, compute_dtype=dt, lora_rank=RANK, lora_alpha=ALPHA, lora_fused=fused)
            net.load_state_dict({**up, **lora})
            outs[fused] = net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample
            e = rel(outs[fused], pred_ref)
            print(f"[{dt}] {'fused' if fused else 'merged'} forward rel-L2 {e:.3e} (<= {tol:.1e})")
            assert e < tol
        assert rel(outs[True], outs[False]) < tol
        assert rel(bare, pred_ref) > tol            # the adapters matter at this bound ...
        assert rel(outs[True], bare) > tol          # ... and the handle applies them
    # three DDIM steps inside the captured graph against the same steps launched eagerly
    sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sched.set_timesteps(3)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True)
    net.load_state_dict({**up, **lora})
    finals = {}
    for use_graph in (True, False):
        lat = x.cuda().clone()
        mrisr.Sampler(net, sched, kind="ddim").run(lat, ctx.cuda(), use_graph=use_graph)
        torch.cuda.synchronize()
        finals[use_graph] = lat
    print(f"sampler graph vs eager rel-L2 {rel(finals[True], finals[False]):.3e}")
    assert rel(finals[True], finals[False]) <= 1e-6
    assert rel(finals[True], x) > 1e-3


PROMPTS = ["", "an axial T2 slice", "an axial T1 slice"]


def test_fit_trains_conv_adapters_and_resumes(tmp_path):
    """mrisr.fit with conv + attention adapters: 4 optimiser steps of 2 micro-batches in the captured graphs equal the eager loop on the
    same batches (1e-6); a resume from checkpoint-2 reproduces steps 3-4; the checkpoint file holds the 4-D keys; a checkpoint with conv
    adapters does not resume into a run without them."""
    import mrisr
    from oracle import unet as ou
    from oracle import vae as ov
    from safetensors.torch import load_file
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=551, perturb_norm=True)
    lin = ffref.init_adapters(up, ffref.block_modules(up, ATTN), RANK, seed=552)
    conv = ref.init_adapters(up, ref.resnet_modules(up), RANK, seed=553)
    lora = {**lin, **conv}
    vp = ov.init_vae_params(ov.TINY_VAE, seed=554)
    g = torch.Generator().manual_seed(555)
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    items = []
    for i in range(8):
        hr = (torch.sin(xx / (3 + i % 7)) * torch.cos(yy / (4 + i % 5)) + 0.1 * torch.randn((64, 64), generator=g)).clamp(-1, 1)
        lr = torch.nn.functional.avg_pool2d(hr[None, None], 4).repeat_interleave(4, 2).repeat_interleave(4, 3)[0]
        items.append({"hr": hr[None], "lr": lr, "txt": PROMPTS[1 + i % 2]})
    embeds = {p: torch.randn((L, cfg.cross_attention_dim), generator=g) for p in PROMPTS}

    def models(adapters):
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=RANK, lora_alpha=ALPHA, lora_fused=True)
        unet.load_state_dict({**up, **adapters})
        vae = mrisr.AutoencoderKL(ov.TINY_VAE, compute_dtype="f32")
        vae.load_state_dict(vp)
        return unet, vae

    def config(out):
        return mrisr.TrainConfig(output_dir=str(out), resolution=64, train_batch_size=2, gradient_accumulation_steps=2, max_train_steps=4,
                                 learning_rate=1e-3, lr_warmup_steps=1, logging_steps=1, validation_steps=1000, checkpointing_steps=2,
                                 mixed_precision="no", proportion_empty_prompts=0.1, seed=78)

    unet, vae = models(lora)
    c = config(tmp_path / "a")
    res = mrisr.fit(c, unet, vae, items, embeds)
    assert res.step == 4 and res.loop.num_captures == 2   # no allocation, tuning or attribute call left for the captures to trip over
    assert [k for k, _, _ in res.trainer.layout] == list(lora)

    unet_e, _ = models(lora)
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
    sd1 = res.trainer.state_dict()
    assert all(not torch.equal(sd1[k].cpu(), lora[k]) for k in conv)

    ck2, ck4 = (os.path.join(str(tmp_path / "a"), f"checkpoint-{n}") for n in (2, 4))
    disk = mrisr.train.lora_keys_from_disk(load_file(os.path.join(ck4, "pytorch_lora_weights.safetensors")))
    assert set(disk) == set(sd1) and all(disk[k].shape == sd1[k].shape and torch.equal(disk[k], sd1[k].cpu()) for k in sd1)
    assert all(disk[k].ndim == 4 for k in conv)
    unet_r, vae_r = models(lora)
    resumed = mrisr.fit(config(tmp_path / "b"), unet_r, vae_r, items, embeds, resume_from=ck2)
    assert resumed.step == 4
    assert rel(resumed.trainer.theta, res.trainer.theta) <= 1e-6
    assert np.abs(resumed.losses[2:] - res.losses[2:]).max() <= 1e-6 * np.abs(res.losses[2:]).max()
    # a run whose adapter set differs does not take this checkpoint
    unet_l, vae_l = models(lin)
    with pytest.raises((ValueError, KeyError)):
        mrisr.fit(config(tmp_path / "c"), unet_l, vae_l, items, embeds, resume_from=ck2)


def test_layout_without_conv_adapters_is_unchanged():
    """Attention adapters only: keys, shapes, offsets and count of the flat vector are what mrisr.params.lora_param_shapes lists, in its
    order (the library's order for these targets), 2-D."""
    import mrisr
    from mrisr import params as P
    from oracle import unet as ou
    cfg = small_cfg()
    up = ou.init_unet_params(cfg, seed=571, perturb_norm=True)
    tmpl = [(k, s) for k, s, _ in P.lora_param_shapes(mrisr.UNetConfig.from_oracle_like(cfg), RANK)]
    lora = P.random_state_dict(P.lora_param_shapes(mrisr.UNetConfig.from_oracle_like(cfg), RANK), seed=572, device="cpu")
    _, tr = trainer(cfg, up, lora, "f32")
    assert [(k, tuple(v.shape)) for k, v in tr.state_dict().items()] == tmpl
    offs = np.cumsum([0] + [s[0] * s[1] for _, s in tmpl])[:-1].tolist()
    assert [(k, o, s) for k, o, s in tr.layout] == [(k, o, s) for (k, s), o in zip(tmpl, offs)]
    assert tr.num_trainable == sum(s[0] * s[1] for _, s in tmpl)
