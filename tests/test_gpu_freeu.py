"""GPU: FreeU (``UNet2DConditionModel.enable_freeu``) in the UNet forward and the graph sampler against the patched CPU oracle
(tests/freeu_ref.py, itself checked by test_freeu_cpu.py): single forwards, "off means off", trajectories, graph == eager, FreeU
together with CFG + PAG, tiles, ControlNet residuals and adapter features, graph captures, the refusals and ``log_validation``.
TINY UNet (+ rank-4 LoRA), B = 2.

Tolerances: those of tests/test_gpu_unet.py - 1e-3 relative L2 for the f32 engine, 5e-2 for bf16; trajectories 1e-3 relative L2 and
max-relative like every f32 sampler test here.  Every setting used moves the oracle's prediction by >= 1e-2 (test_freeu_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import freeu_ref as fr
from pag_ref import PagUNet
from pag_testlib import StubVAE, maxrel, rel
from tiles_ref import TiledUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DOCS = fr.SD15_DOCS
T500 = torch.tensor(500)


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    from oracle import unet as ou
    cfg, p = fr.tiny_params()
    cp = ou.init_controlnet_params(cfg, seed=3302, perturb_norm=True)
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    unet.load_state_dict(p)
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="f32")
    cnet.load_state_dict(cp)
    return dict(cfg=cfg, p=p, unet=unet, cnet=cnet, o_unet=ou.OracleUNet(p, cfg), plain={})


inputs = fr.inputs


def plain_ref(tiny, hw):
    """The oracle's forward without FreeU, once per size."""
    if hw not in tiny["plain"]:
        x, ctx = inputs(tiny["cfg"], hw)
        tiny["plain"][hw] = tiny["o_unet"](x, T500, encoder_hidden_states=ctx).sample
    return tiny["plain"][hw]


def freeu_ref_forward(tiny, hw, vals, **kw):
    x, ctx = inputs(tiny["cfg"], hw)
    with fr.freeu(*vals, tiny["cfg"]):
        return tiny["o_unet"](x, T500, encoder_hidden_states=ctx, **kw).sample


def device_forward(net, cfg, hw, vals, **kw):
    x, ctx = inputs(cfg, hw)
    if vals is not None:
        net.enable_freeu(*vals)
    try:
        out = net(x.cuda(), T500, encoder_hidden_states=ctx.cuda(), **kw).sample
        torch.cuda.synchronize()
    finally:
        net.disable_freeu()
    return out.float().cpu()


def host_scheduler(kind, n):
    import mrisr
    cls = {"ddim": mrisr.DDIMScheduler, "unipc": mrisr.UniPCMultistepScheduler}[kind]
    sp = cls(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    return sp


def captures(smp):
    import mrisr
    return int(mrisr._lib.lib().mrisr_sampler_num_captures(smp._h))


# ------------------------------------------------------------------------------------------------ 1. one forward
@pytest.mark.parametrize("name", ["docs", "s1", "s2", "b1", "b2"])
@pytest.mark.parametrize("hw", [(16, 16), (16, 24)], ids=["16x16", "16x24"])
def test_single_forward_f32(tiny, hw, name):
    vals = DOCS if name == "docs" else fr.SINGLES[name]
    ref = freeu_ref_forward(tiny, hw, vals)
    assert tiny["unet"].freeu is None
    out = device_forward(tiny["unet"], tiny["cfg"], hw, vals)
    r, moved, want = rel(out, ref), rel(out, plain_ref(tiny, hw)), rel(ref, plain_ref(tiny, hw))
    print(f"freeu forward f32 {hw} {name}={vals}: rel {r:.3e}; differs from the plain forward by {moved:.3e} (oracle {want:.3e})")
    assert r <= 1e-3
    assert moved > 10 * 1e-3


@pytest.mark.parametrize("hw", [(16, 16), (16, 24)], ids=["16x16", "16x24"])
def test_single_forward_bf16(tiny, hw):
    import mrisr
    net = mrisr.UNet2DConditionModel(tiny["cfg"], compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    ref = freeu_ref_forward(tiny, hw, DOCS)
    out = device_forward(net, tiny["cfg"], hw, DOCS)
    r, moved = rel(out, ref), rel(out, plain_ref(tiny, hw))
    print(f"freeu forward bf16 {hw} {DOCS}: rel {r:.3e}; differs from the plain forward by {moved:.3e}")
    assert r <= 5e-2


def test_freeu_property_and_disable_is_the_forward_of_before(tiny):
    """After disable_freeu the forward is bit-equal to that of a model that never had FreeU, with the same workspace."""
    import mrisr
    cfg, hw = tiny["cfg"], (16, 16)
    never = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    never.load_state_dict(tiny["p"])
    want = device_forward(never, cfg, hw, None)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    assert net.freeu is None
    net.enable_freeu(*DOCS)
    assert net.freeu == DOCS
    with pytest.raises(AttributeError):
        net.freeu = None  # read-only
    x, ctx = inputs(cfg, hw)
    on = net(x.cuda(), T500, encoder_hidden_states=ctx.cuda()).sample.cpu()
    ws_on = net.workspace_bytes
    net.disable_freeu()
    assert net.freeu is None
    off = device_forward(net, cfg, hw, None)
    assert torch.equal(off, want) and not torch.equal(on, want)
    assert net.workspace_bytes == never.workspace_bytes == ws_on  # FreeU works in place: no activation of its own


# ------------------------------------------------------------------------------------------------ 2. trajectories
def check_states(tag, make_sampler, x0, traj, n, run_kw, tol=1e-3):
    smp = make_sampler()
    for k in range(1, n + 1):
        lat = x0.clone().contiguous()
        smp.set_range(0, k)
        smp.run(lat, **run_kw)
        torch.cuda.synchronize()
        r, m = rel(lat, traj[k]), maxrel(lat, traj[k])
        print(f"{tag}: state {k}/{n} rel {r:.3e} maxrel {m:.3e}")
        assert r < tol and m < tol, (tag, k, r, m)


@pytest.mark.parametrize("kind", ["ddim", "unipc"])
def test_trajectory_and_graph_replay_equals_eager(tiny, kind):
    import mrisr
    import multistep_ref as mref
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, n = tiny["cfg"], 3
    x, ctx = inputs(cfg, (16, 16), 3320)
    sp = host_scheduler(kind, n)
    with fr.freeu(*DOCS, cfg):
        if kind == "ddim":
            so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
            so.set_timesteps(n)
            traj = osa.ddim_sample(tiny["o_unet"], x, ctx, so)
        else:
            traj = mref.multistep_sample(kind, tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, last=n)
    unet = tiny["unet"]
    unet.enable_freeu(*DOCS)
    try:
        check_states(f"freeu {kind}", lambda: mrisr.Sampler(unet, sp, kind=kind), x.cuda(), traj, n, dict(encoder_hidden_states=ctx.cuda()))
        finals = {}
        for use_graph in (True, False):
            lat = x.cuda().clone()
            smp = mrisr.Sampler(unet, sp, kind=kind)
            smp.run(lat, ctx.cuda(), use_graph=use_graph)
            torch.cuda.synchronize()
            finals[use_graph] = lat.cpu()
            assert captures(smp) == (1 if use_graph else 0)
        assert torch.equal(finals[True], finals[False])
    finally:
        unet.disable_freeu()
    plain = x.cuda().clone()
    mrisr.Sampler(unet, sp, kind=kind).run(plain, ctx.cuda())
    torch.cuda.synchronize()
    assert rel(finals[True], plain) > 1e-3  # FreeU was on: the run differs from the plain one by more than the tolerance above


def test_with_cfg_and_pag_on_mid(tiny):
    """CFG + PAG: 3B rows, the perturbed ones get FreeU like the others.  Reference: PagUNet (tests/pag_ref.py) under freeu_ref."""
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n, g, s = tiny["cfg"], 2, 3, 3.0, 2.0
    x, ctx_c = inputs(cfg, (16, 16), 3330)
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), generator=torch.Generator().manual_seed(3331))
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    with fr.freeu(*DOCS, cfg):
        traj = osa.ddim_sample(PagUNet(tiny["o_unet"], ctx_c, s, ("mid",), ctx_u=ctx_u.expand(B, -1, -1), guidance_scale=g), x, None, so)
    sp = host_scheduler("ddim", n)
    kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, pag_scale=s, pag_applied_layers=("mid",))
    tiny["unet"].enable_freeu(*DOCS)
    try:
        check_states("freeu + cfg + pag(mid)", lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), traj, n, kw)
    finally:
        tiny["unet"].disable_freeu()


def test_with_tiles(tiny):
    """16 x 16 canvas, tile 8, overlap 0 (T = 4): every tile is a forward of its own, so the planes are the tiles' (1 x 1 and 2 x 2
    in the two FreeU blocks).  Reference: TiledUNet (tests/tiles_ref.py) under freeu_ref."""
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, n = tiny["cfg"], 3
    x, ctx = inputs(cfg, (16, 16), 3340)
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    with fr.freeu(*DOCS, cfg):
        traj = osa.ddim_sample(TiledUNet(tiny["o_unet"], 16, 16, 8, 0), x, ctx, so)
    sp = host_scheduler("ddim", n)

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_tiles(8, 0)
        return smp

    tiny["unet"].enable_freeu(*DOCS)
    try:
        check_states("freeu + tiles", make, x.cuda(), traj, n, dict(encoder_hidden_states=ctx.cuda()))
    finally:
        tiny["unet"].disable_freeu()


def test_filter_sees_the_residual_carrying_skip(tiny, golden_dir):
    """ControlNet residuals (16 x 16 latents) and adapter features (8 x 8, the golden adapter input): diffusers filters the skip after
    both were added.  The residuals are as large as the skips, so filtering before adding them misses the bound by far."""
    from oracle import adapter as oad
    cfg, hw = tiny["cfg"], (16, 16)
    shapes = tiny["unet"]._skip_shapes(2, *hw)
    g = torch.Generator().manual_seed(3350)
    down = [0.5 * torch.randn(s, generator=g) + 0.5 for s in shapes[:-1]]
    mid = 0.5 * torch.randn(shapes[-1], generator=g)
    ref = freeu_ref_forward(tiny, hw, DOCS, down_block_additional_residuals=down, mid_block_additional_residual=mid)
    out = device_forward(tiny["unet"], cfg, hw, DOCS, down_block_additional_residuals=[d.cuda() for d in down],
                         mid_block_additional_residual=mid.cuda())
    no_res = freeu_ref_forward(tiny, hw, DOCS)
    r = rel(out, ref)
    print(f"freeu + ControlNet residuals: rel {r:.3e}; the residuals move the reference by {rel(ref, no_res):.3e}")
    assert r <= 1e-3 and rel(ref, no_res) > 1e-2
    gold = np.load(os.path.join(golden_dir, "adapter_xl.npz"))
    feats = oad.adapter_forward(oad.init_adapter_params(oad.ADAPTER_TINY, seed=401), oad.ADAPTER_TINY, torch.from_numpy(gold["x"]))
    assert feats[0].shape[0] == 2
    hw = (8, 8)
    ref = freeu_ref_forward(tiny, hw, DOCS, down_intrablock_additional_residuals=[f.clone() for f in feats])
    out = device_forward(tiny["unet"], cfg, hw, DOCS, down_intrablock_additional_residuals=[f.cuda() for f in feats])
    r = rel(out, ref)
    print(f"freeu + adapter features: rel {r:.3e}; the features move the reference by {rel(ref, freeu_ref_forward(tiny, hw, DOCS)):.3e}")
    assert r <= 1e-3


# ------------------------------------------------------------------------------------------------ 3. graph captures
def test_a_changed_value_captures_again_and_a_repeat_does_not(tiny):
    import mrisr
    cfg, unet = tiny["cfg"], tiny["unet"]
    x, ctx = inputs(cfg, (16, 16), 3360)
    sp = host_scheduler("ddim", 3)
    smp = mrisr.Sampler(unet, sp, kind="ddim")

    def run():
        lat = x.cuda().clone()
        smp.run(lat, ctx.cuda())
        torch.cuda.synchronize()
        return lat.cpu()

    try:
        plain = run()
        assert captures(smp) == 1
        unet.enable_freeu(*DOCS)
        a = run()
        assert captures(smp) == 2
        assert torch.equal(run(), a) and captures(smp) == 2          # the same state: the graph is replayed
        unet.enable_freeu(*DOCS)                                     # set again to the same values: still the same state
        assert torch.equal(run(), a) and captures(smp) == 2
        for i in range(4):                                           # each of the four values is part of the key
            vals = list(DOCS)
            vals[i] += 0.25
            unet.enable_freeu(*vals)
            b = run()
            assert captures(smp) == 3 + i and not torch.equal(b, a)
        unet.disable_freeu()
        assert torch.equal(run(), plain) and captures(smp) == 7
    finally:
        unet.disable_freeu()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    cfg = tiny["cfg"]
    x, ctx = inputs(cfg, (16, 16), 3370)
    x, ctx = x.cuda(), ctx.cuda()
    lat = x.clone()
    sp = host_scheduler("ddim", 3)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4, lora_fused=True)
    net.load_state_dict(tiny["p"])
    # the cache first, then FreeU: the run refuses
    cached = mrisr.Sampler(net, sp, kind="ddim")
    cached.set_cache(2, 1)
    net.enable_freeu(*DOCS)
    try:
        with pytest.raises(ValueError, match="cache"):
            cached.run(lat, ctx)
        t_lat, t_e = L.as_tensor(lat), L.as_tensor(ctx.contiguous())
        with pytest.raises(mrisr.MrisrError, match="cache"):  # the C ABI by itself
            L.check(L.lib().mrisr_sampler_run(cached._h, C.byref(t_lat), None, None, C.byref(t_e), None, None, 0, 1, L.stream_ptr()))
        # FreeU first, then the cache: set_cache refuses, in Python and in the C ABI; interval 1 (no cache) is fine
        smp = mrisr.Sampler(net, sp, kind="ddim")
        with pytest.raises(ValueError, match="FreeU"):
            smp.set_cache(2, 1)
        with pytest.raises(mrisr.MrisrError, match="FreeU"):
            L.check(L.lib().mrisr_sampler_set_cache(smp._h, 2, 1))
        smp.set_cache(1, 1)
        # a cached forward and a training step
        cb, cc, ch, cw = net.cache_shape(1, 2, 16, 16)
        with pytest.raises(mrisr.MrisrError, match="feature cache"):
            net.forward_cached(x, T500, ctx, torch.zeros((cb, ch, cw, cc), device="cuda"), 1, False)
    finally:
        net.disable_freeu()
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran on the latents
    # a ControlNet handle; bad values at the C ABI (Python's check_freeu never lets them through)
    f = C.c_float
    with pytest.raises(mrisr.MrisrError, match="ControlNet"):
        L.check(L.lib().mrisr_model_set_freeu(tiny["cnet"]._h, 1, f(0.9), f(0.2), f(1.5), f(1.6)))
    for i, n in enumerate(("s1", "s2", "b1", "b2")):
        for bad in (-1.0, float("nan"), float("inf")):
            vals = [0.9, 0.2, 1.5, 1.6]
            vals[i] = bad
            with pytest.raises(mrisr.MrisrError, match=n):
                L.check(L.lib().mrisr_model_set_freeu(net._h, 1, *[f(v) for v in vals]))
    with pytest.raises(ValueError, match="s2"):
        net.enable_freeu(0.9, -0.2, 1.5, 1.6)
    assert net.freeu is None
    # none of the refused calls left a state behind: the forward is the plain one
    a = net(x, T500, encoder_hidden_states=ctx).sample
    torch.cuda.synchronize()
    assert rel(a.cpu(), tiny["o_unet"](x.cpu(), T500, encoder_hidden_states=ctx.cpu()).sample) <= 1e-3
    # a training step while the state is on
    net.enable_freeu(*DOCS)
    try:
        tr = mrisr.LoRATrainer(net)
        with pytest.raises(mrisr.MrisrError, match="FreeU"):
            tr.forward_backward(x, torch.full((2,), 500, dtype=torch.int64).cuda(), ctx, torch.zeros_like(x))
    finally:
        net.disable_freeu()


# ------------------------------------------------------------------------------------------------ 5. log_validation
def test_log_validation_freeu_restores_the_state(tiny):
    import mrisr
    cfg, n, unet = tiny["cfg"], 3, tiny["unet"]
    gen = torch.Generator().manual_seed(3380)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(128, 128), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    ctx = torch.randn((1, 77, cfg.cross_attention_dim), generator=gen).cuda()
    vae, acc = StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(3381)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(unet, None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx, num_inference_steps=n, **kw))

    try:
        plain = panel()
        got = panel(freeu=DOCS)
        assert unet.freeu is None  # restored
        W = got.shape[1] // 3
        assert not np.array_equal(plain[:, W:2 * W], got[:, W:2 * W])
        assert np.array_equal(plain[:, :W], got[:, :W]) and np.array_equal(plain[:, 2 * W:], got[:, 2 * W:])
        assert np.array_equal(plain, panel())
        assert np.array_equal(plain, panel(freeu=(1.0, 1.0, 1.0, 1.0)))  # x + 0 * t and x * 1: the identity setting changes no bit
        prev = (0.8, 0.3, 1.2, 1.4)
        unet.enable_freeu(*prev)
        own = panel()  # freeu=None: the UNet's own state is used
        assert np.array_equal(got, panel(freeu=DOCS)) and unet.freeu == prev
        assert np.array_equal(own, panel()) and not np.array_equal(own[:, W:2 * W], got[:, W:2 * W])
        with pytest.raises(ValueError, match="cache"):  # an error inside the run: restored as well
            panel(freeu=DOCS, cache_interval=2)
        assert unet.freeu == prev
        with pytest.raises(ValueError, match="b1"):
            panel(freeu=(0.9, 0.2, -1.5, 1.6))
        assert unet.freeu == prev
    finally:
        unet.disable_freeu()
