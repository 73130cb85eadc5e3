"""GPU: DoRA adapters (peft ``use_dora=True``) on the linear targets through the model: the packed layout
(csrc/model.hip::linear - rows of the weight and the B bank scaled by g = m / ||W + s B A||, by csrc/dora.hip), merged
(``lora_fused=False``: W_eff = diag(g)(W + s B A)) and un-merged, eager and in the sampler's captured graph; ``use_rslora``; and training -
the magnitudes in the flat trainable vector, ``dB`` scaled per row, ``dm`` by ``dora_mag_grad`` (csrc/train.hip::linear_bwd), the refresh of
every scaled view after an optimiser step (``dora_refresh_t``), ``LoRATrainer`` and ``fit`` with checkpoints and resume.

TINY (64 / 128 / 256 / 256), B = 2, 8 x 8 latents, seeded weights, lora_alpha = 2 r, the magnitudes perturbed +- 10 % around the row norm
so that g != 1.  Reference: tests/dora_ref.py (adapters and magnitudes folded into float64 weights, the oracle's forward).  Bounds are
those the project applies to LoRA for the same quantities: 1e-3 (f32 engine) and 5e-2 (bf16 engine) for the prediction
(tests/test_gpu_unet.py, tests/test_gpu_lora_highrank.py), 1e-3 for every f32 gradient / AdamW-updated tensor and 6e-2 for the bf16 step
(tests/test_gpu_train.py, tests/test_gpu_lora_ff.py), bit equality of graph replay against eager launches."""
import ctypes as C_
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dora_ref as dref  # noqa: E402
import lora_ff_ref as lref  # noqa: E402

pytestmark = pytest.mark.gpu

B, H, L = 2, 8, 8
ATTN_FF = lref.ATTN + (lref.FF1, lref.FF2)
NINE = "all"  # lora_ff_ref.block_modules: proj_in, attn1 q / k / v, attn1 out, attn2 q, attn2 k / v, attn2 out, ff.net.0.proj, ff.net.2, proj_out
TOL = {"f32": 1e-3, "bf16": 5e-2}   # forward: tests/test_gpu_unet.py::test_unet_forward_matches_oracle
TOL_GRAD = {"f32": 1e-3, "bf16": 6e-2}  # prediction / loss / flat gradient of the step: tests/test_gpu_train.py, tests/test_gpu_lora_ff.py
MAG = dref.MAG


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_batch(cfg, seed, b=B, h=H, ctx_len=L):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, 4, h, h), generator=g)
    ctx = torch.randn((b, ctx_len, cfg.cross_attention_dim), generator=g)
    t = torch.randint(0, 1000, (b,), generator=g)
    return x, t, ctx


def build(cfg, sd, r, dt, fused=True, dora=True, **kw):
    import mrisr
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype=dt, lora_rank=r, lora_alpha=2.0 * r, lora_fused=fused, use_dora=dora, **kw)
    net.load_state_dict(sd)
    return net


def run(net, x, t, ctx):
    return net(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda()).sample


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


def tiny(r, which, seed):
    """TINY + rank-r adapters on `which` + magnitudes 10 % off the norm; the float64 prediction of the reference"""
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=seed, perturb_norm=True)
    lora = lref.init_adapters(up, lref.block_modules(up, which), r, seed=seed + 1)
    mags = dref.init_magnitudes(up, lora, 2.0, perturb=0.1, seed=seed + 2)
    batch = make_batch(cfg, seed + 3)
    with torch.no_grad():
        want = dref.forward(cfg, up, {**lora, **mags}, 2.0, *batch)
        as_lora = lref.forward(cfg, up, lora, 2.0, *batch)
    assert rel(as_lora, want) > 1e-2  # the magnitudes matter: the plain-LoRA function is somewhere else
    return cfg, up, lora, mags, batch, want


@pytest.fixture(scope="module")
def nine4():
    return tiny(4, NINE, 1950)


@pytest.mark.parametrize("r,which", [(4, lref.ATTN), (32, lref.ATTN), (4, NINE), (32, NINE), (8, ATTN_FF)],
                         ids=["r4-attn", "r32-attn", "r4-nine", "r32-nine", "r8-attn-ff"])
def test_forward_matches_the_reference_merged_and_unmerged(r, which):
    cfg, up, lora, mags, batch, want = tiny(r, which, 1900 + r + len(which))
    sd = {**up, **lora, **mags}
    for dt in ("f32", "bf16"):
        fused = run(build(cfg, sd, r, dt, True), *batch)
        merged = run(build(cfg, sd, r, dt, False), *batch)
        print(f"[{dt} r={r}] un-merged vs reference {rel(fused, want):.3e}, merged vs reference {rel(merged, want):.3e}, "
              f"un-merged vs merged {rel(fused, merged):.3e} (<= {TOL[dt]:.0e})")
        assert rel(fused, want) < TOL[dt] and rel(merged, want) < TOL[dt]
        assert rel(fused, merged) < TOL[dt]


def test_packing_runs_the_dora_kernel_and_plain_lora_does_not(nine4):
    cfg, up, lora, mags, batch, _ = nine4
    import mrisr
    for fused in (True, False):
        net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=8.0, lora_fused=fused, use_dora=True)
        assert "dora_scale" in prof(lambda: net.load_state_dict({**up, **lora, **mags}))
    # use_dora=False: the load, a rank-4 forward and a training step launch no dora* class, and the trainable layout is today's
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=8.0, lora_fused=True)
    names = prof(lambda: net.load_state_dict({**up, **lora}))
    names |= prof(lambda: run(net, *batch))
    tr = mrisr.LoRATrainer(net)
    tgt = torch.randn((B, 4, H, H), generator=torch.Generator().manual_seed(5))
    x, t, ctx = batch
    names |= prof(lambda: tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda()))
    assert names and not any(n.startswith("dora") for n in names), sorted(names)
    assert [k for k, _, _ in tr.layout] == list(lora)
    off = 0
    for (k, o, shp), v in zip(tr.layout, lora.values()):
        assert o == off and tuple(shp) == tuple(v.shape), k
        off += v.numel()
    assert off == tr.num_trainable


def test_initial_magnitude_reproduces_the_plain_lora_forward(nine4):
    import mrisr
    cfg, up, lora, _, batch, _ = nine4
    m0 = mrisr.dora_magnitude_init(up, lora, 2.0)
    plain = run(build(cfg, {**up, **lora}, 4, "f32", True, dora=False), *batch)
    for fused in (True, False):
        d = rel(run(build(cfg, {**up, **lora, **m0}, 4, "f32", fused), *batch), plain)
        print(f"[f32] DoRA at m = ||W + s B A|| vs plain LoRA ({'un-merged' if fused else 'merged'}): rel-L2 {d:.3e} (<= 1e-3)")
        assert d < TOL["f32"]


def test_real_width_rank_4_keeps_the_fused_routes_consistent():
    """320 / 640 channels, r = 4: the C = 320 blocks run the fused middle / feed-forward kernels on K-permuted copies of the weights
    (q2p, out2p, ff2p, proj_outp), which are packed from the scaled rows: a copy that missed the scale shows here"""
    from oracle import unet as ou
    cfg = ou.UNetConfig(block_out_channels=(320, 640), attn_levels=(True, True), cross_attention_dim=64)
    up = ou.init_unet_params(cfg, seed=1971, perturb_norm=True)
    lora = lref.init_adapters(up, lref.block_modules(up, lref.ATTN), 4, seed=1972)
    mags = dref.init_magnitudes(up, lora, 2.0, perturb=0.1, seed=1973)
    x, t, ctx = make_batch(cfg, 1974, b=1, h=16, ctx_len=77)
    with torch.no_grad():
        want = dref.forward(cfg, up, {**lora, **mags}, 2.0, x, t, ctx)
    sd = {**up, **lora, **mags}
    for dt in ("f32", "bf16"):
        fused, merged = run(build(cfg, sd, 4, dt, True), x, t, ctx), run(build(cfg, sd, 4, dt, False), x, t, ctx)
        print(f"[{dt}] 320 / 640, r = 4: un-merged {rel(fused, want):.3e}, merged {rel(merged, want):.3e} (<= {TOL[dt]:.0e})")
        assert rel(fused, want) < TOL[dt] and rel(merged, want) < TOL[dt]


def test_sampler_graph_equals_eager(nine4):
    import mrisr
    cfg, up, lora, mags, (x, _, ctx), _ = nine4
    for dt in ("f32", "bf16"):
        net = build(cfg, {**up, **lora, **mags}, 4, dt)
        finals = {}
        for graph in (True, False):
            sched = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
            sched.set_timesteps(5)
            lat = x.cuda().clone().contiguous()
            mrisr.Sampler(net, sched, kind="ddim").run(lat, ctx.cuda(), use_graph=graph)
            torch.cuda.synchronize()
            finals[graph] = lat.float().cpu()
        assert bool(torch.isfinite(finals[True]).all()) and torch.equal(finals[True], finals[False]), dt


def test_rslora_equals_the_alpha_that_gives_the_same_scale():
    """r = 16, lora_alpha = 32: rsLoRA's scale 32 / sqrt(16) = 8 is that of lora_alpha = 128 without it - bit for bit"""
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=1981, perturb_norm=True)
    lora = lref.init_adapters(up, lref.block_modules(up, ATTN_FF), 16, seed=1982)
    batch = make_batch(cfg, 1983)
    outs = []
    for kw in (dict(lora_alpha=32.0, use_rslora=True), dict(lora_alpha=128.0)):
        net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=16, lora_fused=True, **kw)
        assert net.lora_scale == 8.0
        net.load_state_dict({**up, **lora})
        outs.append(run(net, *batch))
    assert torch.equal(outs[0], outs[1])
    plain = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=16, lora_alpha=32.0, lora_fused=True)
    plain.load_state_dict({**up, **lora})
    assert not torch.equal(run(plain, *batch), outs[0])


def test_state_dict_checks_and_the_trainer(nine4):
    import mrisr
    cfg, up, lora, mags, batch, _ = nine4
    # refused before the first parameter is pushed
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=8.0)
    with pytest.raises(ValueError, match="use_dora=True"):
        net.load_state_dict({**up, **lora, **mags})
    assert not net._params and not net._finalized
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=8.0, use_dora=True)
    km = next(iter(mags))
    with pytest.raises(ValueError, match="without"):
        net.load_state_dict({**up, **lora, **{k: v for k, v in mags.items() if k != km}})
    assert not net._params and not net._finalized
    # peft's on-disk spelling loads, and gives the same bits
    from mrisr.train import lora_keys_to_disk
    a = run(build(cfg, {**up, **lora, **mags}, 4, "f32"), *batch)
    b = run(build(cfg, {**up, **lora_keys_to_disk({**lora, **mags}, "peft")}, 4, "f32"), *batch)
    assert torch.equal(a, b)
    # the handle itself refuses what the host check would have caught (a caller of the C ABI that never called mrisr_model_set_dora)
    from mrisr import _lib as L_
    raw = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=8.0)
    with pytest.raises(L_.MrisrError, match="DoRA"):
        for k, v in {**up, **lora, **mags}.items():
            L_.push_param(L_.lib().mrisr_model_set_param, raw._h, k, v)
        L_.check(L_.lib().mrisr_model_finalize(raw._h, L_.stream_ptr()))


# ---- training: LoRATrainer and fit ---------------------------------------------------------------------------------------------------
def target(seed, b=B, h=H):
    return torch.randn((b, 4, h, h), generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def step4(nine4):
    """the float64 step of the reference on the shared rank-4 model: all nine linears of every block carry DoRA adapters - proj_in, fused
    Q/K/V, attn2.to_k / to_v on the context rows, to_out.0 (bias + residual), ff.net.0.proj, ff.net.2 and proj_out (bias + the block's
    input as residual)"""
    cfg, up, lora, mags, (x, t, ctx), _ = nine4
    tgt = target(1960)
    pred, loss, grads = dref.loss_and_grads(cfg, up, {**lora, **mags}, 2.0, x, t, ctx, tgt)
    return tgt, pred, loss, grads


def test_trainable_layout_puts_the_magnitudes_last(nine4):
    import mrisr
    cfg, up, lora, mags, _, _ = nine4
    tr = mrisr.LoRATrainer(build(cfg, {**up, **lora, **mags}, 4, "f32"))
    keys = [k for k, _, _ in tr.layout]
    assert keys[: len(lora)] == list(lora) and set(keys[len(lora):]) == set(mags) and len(keys) == len(lora) + len(mags)
    off = 0
    for k, o, shp in tr.layout:
        want = tuple(lora[k].shape) if k in lora else tuple(mags[k].shape)
        assert o == off and tuple(shp) == want and (len(shp) == 1) == (k in mags), k
        off += int(np.prod(shp))
    assert off == tr.theta.numel()
    sd = tr.state_dict()
    assert all(torch.equal(sd[k].cpu(), mags[k]) for k in mags) and set(tr.gradients()) == set(keys)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gradients_match_autograd(nine4, step4, dt):
    import mrisr
    cfg, up, lora, mags, (x, t, ctx), _ = nine4
    tgt, pred_ref, loss_ref, gref = step4
    tr = mrisr.LoRATrainer(build(cfg, {**up, **lora, **mags}, 4, dt))
    tr.zero_grad()
    names = prof(lambda: tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda()))
    assert "dora_mag_grad" in names, sorted(names)
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    flat_ref = torch.cat([gref[k].reshape(-1) for k, _, _ in tr.layout])
    print(f"[{dt}] pred {rel(pred, pred_ref):.3e}, loss {float(loss):.6f} vs {loss_ref:.6f}, flat gradient rel-L2 {rel(tr.grad, flat_ref):.3e} (<= {TOL_GRAD[dt]:.0e})")
    assert rel(pred, pred_ref) < TOL_GRAD[dt] and abs(float(loss) - loss_ref) / loss_ref < TOL_GRAD[dt]
    assert rel(tr.grad, flat_ref) < TOL_GRAD[dt]
    grads = tr.gradients()
    if dt == "f32":
        worst = max((rel(grads[k], gref[k]), k) for k in gref)
        print(f"[f32] worst gradient tensor {worst}")
        assert worst[0] < 1e-3, worst
        for kind in (".lora_A.", ".lora_B.", MAG):
            print(f"[f32] worst {kind}: {max((rel(grads[k], gref[k]), k) for k in gref if kind in k)}")
    # ff.net.0.proj: dm and dB per half (value rows, then gate rows - raw order out of the interleaved columns).  f32: every tensor's half
    # at the per-tensor bound.  bf16: the bound of the bf16 step is one for a flat bucket (no test of the project holds a single bf16
    # gradient tensor to it: the mid block's sum over B * 1 tokens is rounding noise, 6.7e-2 measured on its gate rows where the f32
    # engine has 6e-6), so each half is checked as the bucket of that half of every block
    for kind in (".lora_B.", MAG):
        keys = [k for k in gref if lref.FF1 in k and kind in k]
        assert keys
        for name, sl in (("value", lambda v: v[: v.shape[0] // 2]), ("gate", lambda v: v[v.shape[0] // 2:])):
            if dt == "f32":
                for k in keys:
                    assert rel(sl(grads[k]), sl(gref[k])) < 1e-3, (k, name)
            d = rel(torch.cat([sl(grads[k]).reshape(-1) for k in keys]), torch.cat([sl(gref[k]).reshape(-1) for k in keys]))
            print(f"[{dt}] ff.net.0.proj {kind} {name} halves, all blocks: rel-L2 {d:.3e} (<= {TOL_GRAD[dt]:.0e})")
            assert d < TOL_GRAD[dt], (kind, name, d)


def test_gradients_match_autograd_rank_32():
    """the packed high-rank layout on all nine linears (proj_in / proj_out included): [W | sB] rows and sB columns scaled, dB through
    lora_wgrad_hr into scratch; f32, every tensor"""
    import mrisr
    cfg, up, lora, mags, (x, t, ctx), _ = tiny(32, NINE, 1940)
    tgt = target(1944)
    pred_ref, loss_ref, gref = dref.loss_and_grads(cfg, up, {**lora, **mags}, 2.0, x, t, ctx, tgt)
    tr = mrisr.LoRATrainer(build(cfg, {**up, **lora, **mags}, 32, "f32"))
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    grads = tr.gradients()
    worst = max((rel(grads[k], gref[k]), k) for k in gref)
    print(f"[f32 r=32] pred {rel(pred, pred_ref):.3e}, loss {float(loss):.6f} vs {loss_ref:.6f}, worst gradient tensor {worst}")
    assert rel(pred, pred_ref) < 1e-3 and abs(float(loss) - loss_ref) / loss_ref < 1e-3 and worst[0] < 1e-3, worst


def test_real_width_rank_4_trains_and_the_refresh_equals_a_fresh_pack():
    """320 / 640 channels, bf16, r = 4 on the attention targets: the step against float64 autograd (bounds of the bf16 step), and - the
    C = 320 blocks run the fused middle on q2p / out2p - a refresh from changed magnitudes gives the bits of a model packed from them"""
    import mrisr
    from oracle import unet as ou
    cfg = ou.UNetConfig(block_out_channels=(320, 640), attn_levels=(True, True), cross_attention_dim=64)
    up = ou.init_unet_params(cfg, seed=1976, perturb_norm=True)
    lora = lref.init_adapters(up, lref.block_modules(up, lref.ATTN), 4, seed=1977)
    mags = dref.init_magnitudes(up, lora, 2.0, perturb=0.1, seed=1978)
    x, t, ctx = make_batch(cfg, 1979, b=1, h=16, ctx_len=77)
    tgt = target(1980, b=1, h=16)
    pred_ref, loss_ref, gref = dref.loss_and_grads(cfg, up, {**lora, **mags}, 2.0, x, t, ctx, tgt)
    net = build(cfg, {**up, **lora, **mags}, 4, "bf16")
    tr = mrisr.LoRATrainer(net)
    tr.zero_grad()
    loss, pred = tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda(), return_pred=True)
    flat_ref = torch.cat([gref[k].reshape(-1) for k, _, _ in tr.layout])
    mag_got = torch.cat([tr.gradients()[k].reshape(-1) for k in mags])
    mag_ref = torch.cat([gref[k].reshape(-1) for k in mags])
    print(f"[bf16 r=4, 320 / 640] pred {rel(pred, pred_ref):.3e}, flat gradient {rel(tr.grad, flat_ref):.3e}, magnitudes alone {rel(mag_got, mag_ref):.3e} (<= 6e-2)")
    assert rel(pred, pred_ref) < TOL_GRAD["bf16"] and rel(tr.grad, flat_ref) < TOL_GRAD["bf16"] and rel(mag_got, mag_ref) < TOL_GRAD["bf16"]
    mags2 = dref.init_magnitudes(up, lora, 2.0, perturb=0.2, seed=1981)
    before = run(net, x, t, ctx)
    tr.load_state_dict(mags2)
    after = run(net, x, t, ctx)
    fresh = run(build(cfg, {**up, **lora, **mags2}, 4, "bf16"), x, t, ctx)
    assert not torch.equal(after, before) and torch.equal(after, fresh)


def test_two_backwards_accumulate_the_sum_of_the_two_references(nine4, step4):
    """no zero_grad between two forward_backward calls on different batches: a row scale applied to the ACCUMULATED dB shows here"""
    import mrisr
    cfg, up, lora, mags, (x, t, ctx), _ = nine4
    tgt, _, _, g1 = step4
    x2, t2, ctx2 = make_batch(cfg, 1961)
    tgt2 = target(1962)
    _, _, g2 = dref.loss_and_grads(cfg, up, {**lora, **mags}, 2.0, x2, t2, ctx2, tgt2)
    tr = mrisr.LoRATrainer(build(cfg, {**up, **lora, **mags}, 4, "f32"))
    tr.zero_grad()
    tr.forward_backward(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda())
    tr.forward_backward(x2.cuda(), t2.cuda(), ctx2.cuda(), tgt2.cuda())
    grads = tr.gradients()
    worst = max((rel(grads[k], g1[k] + g2[k]), k) for k in g1)
    print(f"two accumulated backwards: worst tensor {worst}")
    assert worst[0] < 1e-3, worst


def test_two_optimizer_steps_match_adamw_and_the_forward_uses_the_new_scale(nine4, step4):
    """Two clip + AdamW steps on all nine linears against torch.optim.AdamW + clip_grad_norm_ on the reference, every tensor <= 1e-3.

    AdamW's eps is 1e-6 here, for both sides.  Adam divides every element by its own magnitude, so an element whose true gradient is below
    the f32 noise of its tensor gets an update of order lr from the noise alone unless eps is well above that noise.  With torch's default
    1e-8 that happened to ONE of 1024 elements of down_blocks.2.attentions.0.proj_in.lora_B: true gradient 1.9e-11, device 2.5e-9 (7e-6 of
    the tensor's median |g| = 3.5e-4, the size of the f32 gradient error everywhere), update 2.0e-3 against 1.9e-5, and that element alone
    put the tensor at 2.8e-3; every other tensor was within 1.7e-4.  eps = 1e-6 is 400 x that noise and 1 / 350 of the median gradient,
    so the step is still Adam's and the comparison measures the step, not one zero crossing."""
    import mrisr
    cfg, up, lora, mags, (x, t, ctx), _ = nine4
    tgt = step4[0]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-6, max_grad_norm=1.0)
    net = build(cfg, {**up, **lora, **mags}, 4, "f32")
    tr = mrisr.LoRATrainer(net, **kw)
    lp = dref.leaves({**lora, **mags})
    opt = torch.optim.AdamW(list(lp.values()), lr=kw["lr"], betas=kw["betas"], weight_decay=kw["weight_decay"], eps=kw["eps"])
    for step in range(2):
        opt.zero_grad()
        with torch.enable_grad():  # the row norm is recomputed from the updated A, B inside dref.merged
            loss_ref = torch.nn.functional.mse_loss(dref.forward(cfg, up, lp, 2.0, x, t, ctx), tgt.double())
            loss_ref.backward()
        torch.nn.utils.clip_grad_norm_(list(lp.values()), 1.0)
        opt.step()
        loss = tr.step(x.cuda(), t.cuda(), ctx.cuda(), tgt.cuda())
        sd = tr.state_dict()
        worst = max((rel(sd[k], lp[k]), k) for k in lp)
        print(f"step {step}: loss {float(loss):.6f} vs {float(loss_ref.detach()):.6f}; worst updated tensor {worst}")
        assert abs(float(loss) - float(loss_ref.detach())) / float(loss_ref.detach()) < 1e-3
        assert worst[0] < 1e-3, worst
    with torch.no_grad():
        want = dref.forward(cfg, up, {k: v.detach() for k, v in lp.items()}, 2.0, x, t, ctx)
        stale = dref.forward(cfg, up, {**lora, **mags}, 2.0, x, t, ctx)
    got = run(net, x, t, ctx)
    print(f"post-step forward rel-L2 {rel(got, want):.3e}; against the parameters before the steps {rel(got, stale):.3e}")
    assert rel(got, want) < 1e-3 and rel(got, stale) > 4 * rel(got, want)


@pytest.mark.parametrize("r", [32, 4])
def test_fit_equals_the_hand_driven_trainer_checkpoints_and_resumes(tmp_path, r):
    """Six steps of fit (graphs M and O, the DoRA refresh captured in O) against the hand-driven LoRATrainer on the same batches.

    r = 32: EXACT equality of theta and of the losses (no kernel of that f32 step uses float atomics).  r = 4: within the 1e-6 of
    tests/test_gpu_fit.py, because the rank-4 lora_wgrad folds through LDS float atomics.  The checkpoint round trip
    is bit for bit at both ranks."""
    import mrisr
    from oracle import unet as ou
    from oracle import vae as ov
    from safetensors.torch import load_file
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=1991, perturb_norm=True)
    lora = lref.init_adapters(up, lref.block_modules(up, NINE), r, seed=1992)
    mags = dref.init_magnitudes(up, lora, 2.0, perturb=0.1, seed=1993)
    vp = ov.init_vae_params(ov.TINY_VAE, seed=1994)
    g = torch.Generator().manual_seed(1995)
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    prompts = ["", "an axial T2 slice", "an axial T1 slice"]
    items = []
    for i in range(8):
        hr = (torch.sin(xx / (3 + i % 7)) * torch.cos(yy / (4 + i % 5)) + 0.1 * torch.randn((64, 64), generator=g)).clamp(-1, 1)
        lr = torch.nn.functional.avg_pool2d(hr[None, None], 4).repeat_interleave(4, 2).repeat_interleave(4, 3)[0]
        items.append({"hr": hr[None], "lr": lr, "txt": prompts[1 + i % 2]})
    embeds = {p: torch.randn((L, cfg.cross_attention_dim), generator=g) for p in prompts}

    def models():
        unet = build(cfg, {**up, **lora, **mags}, r, "f32")
        vae = mrisr.AutoencoderKL(ov.TINY_VAE, compute_dtype="f32")
        vae.load_state_dict(vp)
        return unet, vae

    def config(out):
        return mrisr.TrainConfig(output_dir=str(out), resolution=64, train_batch_size=2, gradient_accumulation_steps=1, max_train_steps=6,
                                 learning_rate=1e-3, lr_warmup_steps=1, logging_steps=1, validation_steps=1000, checkpointing_steps=3,
                                 mixed_precision="no", proportion_empty_prompts=0.1, seed=79)

    c = config(tmp_path / "a")
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
    if r == 32:
        assert torch.equal(res.trainer.theta, tr.theta) and np.array_equal(res.losses, losses)
    else:
        assert rel(res.trainer.theta, tr.theta) <= 1e-6 and np.abs(res.losses - losses).max() <= 1e-6 * np.abs(losses).max()
    sd = res.trainer.state_dict()
    assert all(not torch.equal(sd[k].cpu(), mags[k]) for k in mags)  # the magnitudes trained
    # the checkpoint holds the magnitudes under peft's on-disk keys, and reproduces the forward bit for bit
    ck3, ck6 = (os.path.join(str(tmp_path / "a"), f"checkpoint-{n}") for n in (3, 6))
    raw = load_file(os.path.join(ck6, "pytorch_lora_weights.safetensors"))
    assert sum(k.endswith(".lora_magnitude_vector.weight") for k in raw) == len(mags)
    disk = mrisr.train.lora_keys_from_disk(raw)
    assert set(disk) == set(sd) and all(torch.equal(disk[k], sd[k].cpu()) for k in sd)
    x, t, ctx = make_batch(cfg, 1996)
    want = run(unet, x, t, ctx)
    fresh = build(cfg, {**up, **disk}, r, "f32")
    assert torch.equal(run(fresh, x, t, ctx), want)
    # the run resumed from step 3 reproduces the tail
    unet_r, vae_r = models()
    resumed = mrisr.fit(config(tmp_path / "b"), unet_r, vae_r, items, embeds, resume_from=ck3)
    assert resumed.step == 6
    print(f"resumed vs uninterrupted: theta {rel(resumed.trainer.theta, res.trainer.theta):.3e}")
    if r == 32:
        assert torch.equal(resumed.trainer.theta, res.trainer.theta)
        assert np.array_equal(np.asarray(resumed.losses[3:]), np.asarray(res.losses[3:]))
    else:
        assert rel(resumed.trainer.theta, res.trainer.theta) <= 1e-6
        assert np.abs(np.asarray(resumed.losses[3:]) - np.asarray(res.losses[3:])).max() <= 1e-6 * np.abs(res.losses).max()
