"""GPU: the DeepCache-style feature cache - one forward at every depth (store == the plain forward, shallow from its own cache ==
the plain forward, the cache tensor itself), a stale cache, cached trajectories of the step kinds against the oracle loops driven by
tests/deepcache_ref.CachedUNet (itself checked by test_deepcache_cpu.py), graph == eager, the sampler's state, the errors,
``log_validation`` and one SD-1.5-width case.  TINY with rank-4 LoRA, 16 x 16 latents, f32 engine unless stated.

Tolerances are the project's own: f32 1e-3 relative L2 and max-relative against the reference; bf16 5e-2 (a bf16 step as in
test_gpu_guidance.py: the state a step leaves and the prediction it consumed, recovered from that state)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import multistep_ref as mref
from deepcache_ref import CachedUNet, cached_forward, num_skips
from guidance_ref import GuidedUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HW = 16


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def maxrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=4201, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=4203))
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    unet.load_state_dict(p)
    return dict(cfg=cfg, p=p, unet=unet, o_unet=ou.OracleUNet(p, cfg), n=num_skips(cfg))


@pytest.fixture(scope="module")
def tiny_bf16(tiny):
    import mrisr
    net = mrisr.UNet2DConditionModel(tiny["cfg"], compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    return net


def inputs(cfg, B, seed, hw=HW):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, hw, hw), generator=g)
    ctx = torch.randn((B, 77, cfg.cross_attention_dim), generator=g)
    feats = [0.5 * torch.randn((B, c, hw >> i, hw >> i), generator=g) for i, c in enumerate(cfg.block_out_channels)]
    return x, ctx, feats


def new_cache(net, depth, B, hw=HW, fill=float("nan")):
    b, c, h, w = net.cache_shape(depth, B, hw, hw)
    return torch.full((b, h, w, c), fill, dtype=net.compute_dtype, device="cuda")


def dd_scheduler(n):
    import mrisr
    from oracle import schedulers as osch
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    return so, sp


def check_states(tag, make_sampler, x0, traj, n, run_kw):
    """Every state of the n-step cached run (set_range(0, k) stops the fused loop after k steps; the schedule of full and shallow
    steps counts from the range's first step, 0 here) against the reference trajectory."""
    assert len(traj) == n + 1
    smp = make_sampler()
    for k in range(1, n + 1):
        lat = x0.clone().contiguous()
        smp.set_range(0, k)
        smp.run(lat, **run_kw)
        torch.cuda.synchronize()
        r, m = rel(lat, traj[k]), maxrel(lat, traj[k])
        print(f"{tag}: state {k}/{n} rel {r:.3e} maxrel {m:.3e}")
        assert r < 1e-3 and m < 1e-3, (tag, k, r, m)


# ------------------------------------------------------------------------------------------------ 1. one forward, every depth
def test_one_forward_every_depth_with_adapter_features(tiny):
    cfg, net, n = tiny["cfg"], tiny["unet"], tiny["n"]
    B = 2
    x, ctx, feats = inputs(cfg, B, 4301)
    t = torch.tensor(601)
    xd, cd, fd = x.cuda(), ctx.cuda(), [f.cuda() for f in feats]
    plain = net(xd, t.cuda(), encoder_hidden_states=cd, down_intrablock_additional_residuals=fd).sample
    again = net(xd, t.cuda(), encoder_hidden_states=cd, down_intrablock_additional_residuals=fd).sample
    exact = torch.equal(plain, again)
    print(f"two plain forwards of one input are bit-identical: {exact}")

    def same(a, tag):
        if exact:
            assert torch.equal(a, plain), tag
        else:
            assert rel(a, plain) <= 1e-6, (tag, rel(a, plain))

    assert n == 12 and net.cache_shape(1, B, HW, HW) == (B, 64, 16, 16) and net.cache_shape(11, B, HW, HW) == (B, 256, 2, 2)
    for d in range(1, n):
        ref_eps, ref_cache = cached_forward(tiny["p"], cfg, x, t, ctx, d, intrablock=[f.clone() for f in feats])
        cache = new_cache(net, d, B)
        stored = net.forward_cached(xd, t.cuda(), cd, cache, d, False, down_intrablock_additional_residuals=fd)
        same(stored, ("store", d))
        assert bool(torch.isfinite(cache).all()), d
        kept = cache.clone()
        shallow = net.forward_cached(xd, t.cuda(), cd, cache, d, True, down_intrablock_additional_residuals=fd)
        same(shallow, ("shallow", d))
        assert torch.equal(cache, kept), d  # a shallow forward only reads it
        got = cache.permute(0, 3, 1, 2)
        assert tuple(got.shape) == tuple(ref_cache.shape), (d, got.shape, ref_cache.shape)
        r, m, re = rel(got, ref_cache), maxrel(got, ref_cache), rel(shallow, ref_eps)
        print(f"depth {d:2d}: cache {tuple(ref_cache.shape)} rel {r:.3e} maxrel {m:.3e}; shallow eps vs reference rel {re:.3e}")
        assert r < 1e-3 and m < 1e-3 and re < 1e-3 and maxrel(shallow, ref_eps) < 1e-3, (d, r, m, re)


# ------------------------------------------------------------------------------------------------ 2. a stale cache
@pytest.mark.parametrize("dt,B,depth", [("f32", 2, 2), ("bf16", 2, 3), ("f32", 3, 6)])
def test_shallow_forward_from_a_stale_cache(tiny, tiny_bf16, dt, B, depth):
    """The cache of (x, t = 500) under a shallow forward at (x', t = 480): what a cached sampler step computes."""
    cfg = tiny["cfg"]
    net = tiny["unet"] if dt == "f32" else tiny_bf16
    tol = 1e-3 if dt == "f32" else 5e-2
    x, ctx, _ = inputs(cfg, B, 4311 + B)
    x2 = x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(4313))
    _, ref_cache = cached_forward(tiny["p"], cfg, x, torch.tensor(500), ctx, depth)
    ref, _ = cached_forward(tiny["p"], cfg, x2, torch.tensor(480), ctx, depth, cache=ref_cache)
    fresh = tiny["o_unet"](x2, torch.tensor(480), encoder_hidden_states=ctx).sample
    assert rel(ref, fresh) > 10 * tol or dt == "bf16"  # (f32: the stale cache shows well above the tolerance)
    cache = new_cache(net, depth, B)
    net.forward_cached(x.cuda(), torch.tensor(500).cuda(), ctx.cuda(), cache, depth, False)
    out = net.forward_cached(x2.cuda(), torch.tensor(480).cuda(), ctx.cuda(), cache, depth, True)
    r, m = rel(out, ref), maxrel(out, ref)
    print(f"stale cache [{dt}, B={B}, depth {depth}]: rel {r:.3e} maxrel {m:.3e}; stale vs fresh in the reference {rel(ref, fresh):.3e}")
    assert r < tol and (dt == "bf16" or m < tol), (r, m)


# ------------------------------------------------------------------------------------------------ 3. trajectories
@pytest.mark.parametrize("depth", [1, 2])
def test_cached_ddim_trajectory(tiny, depth):
    import mrisr
    from oracle import sampler as osa
    cfg, B, n = tiny["cfg"], 2, 6
    x, ctx, _ = inputs(cfg, B, 4321)
    so, sp = dd_scheduler(n)
    ref_net = CachedUNet(tiny["p"], cfg, 3, depth)
    traj = osa.ddim_sample(ref_net, x, ctx, so)
    assert ref_net.kinds == ["full", "shallow", "shallow"] * 2

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_cache(3, depth)
        return smp

    check_states(f"ddim interval 3 depth {depth}", make, x.cuda(), traj, n, dict(encoder_hidden_states=ctx.cuda()))
    if depth == 1:  # the cache is really in use: the cached device run is not the uncached device run
        a, b = x.cuda().clone(), x.cuda().clone()
        make().run(a, ctx.cuda())
        mrisr.Sampler(tiny["unet"], sp, kind="ddim").run(b, ctx.cuda())
        torch.cuda.synchronize()
        r = rel(a, b)
        print(f"ddim interval 3 depth 1: cached vs uncached device run rel {r:.3e}")
        assert r >= 5e-3, r


def test_cached_res_srdiff_trajectory_with_anchor_and_noise(tiny):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n = tiny["cfg"], 2, 5
    _, ctx, _ = inputs(cfg, B, 4331)
    gen = torch.Generator().manual_seed(4332)
    lr_lat = 0.18215 * torch.randn((B, 4, HW, HW), generator=gen)
    init_noise = torch.randn(lr_lat.shape, generator=gen)
    step_noise = torch.stack([torch.randn(lr_lat.shape, generator=gen) for _ in range(n - 1)])
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    traj = osa.res_srdiff_sample(CachedUNet(tiny["p"], cfg, 2, 3), None, lr_lat, ctx, None, so.timesteps, so.alphas_cumprod, init_noise,
                                 list(step_noise))
    sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, init_noise.cuda())
    assert rel(x0, traj[0]) < 1e-5

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="resshift")
        smp.set_cache(2, 3)
        return smp

    check_states("res-srdiff interval 2 depth 3", make, x0, traj, n,
                 dict(encoder_hidden_states=ctx.cuda(), lr_latents=lr_lat.cuda(), step_noise=step_noise.cuda()))


def test_cached_unipc_trajectory(tiny):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 5
    x, ctx, _ = inputs(cfg, B, 4341)
    sp = mrisr.UniPCMultistepScheduler(timestep_spacing="leading", steps_offset=1, solver_order=2)
    sp.set_timesteps(n)
    traj = mref.multistep_sample("unipc", CachedUNet(tiny["p"], cfg, 2, 1), x, ctx, sp.timesteps, sp.alphas_cumprod, solver_order=2)

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="unipc")
        smp.set_cache(2, 1)
        return smp

    check_states("unipc-2 interval 2 depth 1", make, x.cuda(), traj, n, dict(encoder_hidden_states=ctx.cuda()))


def test_cached_guided_ddim_trajectory(tiny):
    """2B rows per forward: the sampler's cache has 2B rows too, one per (context, sample)."""
    import mrisr
    from oracle import sampler as osa
    cfg, B, n, g, phi = tiny["cfg"], 2, 5, 3.5, 0.7
    x, ctx_c, _ = inputs(cfg, B, 4351)
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), generator=torch.Generator().manual_seed(4352))
    so, sp = dd_scheduler(n)
    ref_net = CachedUNet(tiny["p"], cfg, 2, 1, calls_per_step=2)
    traj = osa.ddim_sample(GuidedUNet(ref_net, ctx_u.expand(B, -1, -1), ctx_c, g, phi), x, None, so)
    assert ref_net.kinds == ["full", "full", "shallow", "shallow"] * 2 + ["full", "full"]

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_cache(2, 1)
        return smp

    check_states("guided ddim interval 2 depth 1", make, x.cuda(), traj, n,
                 dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi))


def test_cached_ddim_trajectory_with_adapter_features(tiny):
    import mrisr
    from oracle import sampler as osa
    cfg, B, n = tiny["cfg"], 2, 5
    x, ctx, feats = inputs(cfg, B, 4361)
    so, sp = dd_scheduler(n)
    traj = osa.ddim_sample(CachedUNet(tiny["p"], cfg, 2, 2), x, ctx, so, intrablock=feats)
    bare = osa.ddim_sample(CachedUNet(tiny["p"], cfg, 2, 2), x, ctx, so)
    assert rel(traj[-1], bare[-1]) > 1e-2  # the features matter

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_cache(2, 2)
        return smp

    check_states("ddim+adapter interval 2 depth 2", make, x.cuda(), traj, n,
                 dict(encoder_hidden_states=ctx.cuda(), adapter_features=[f.cuda() for f in feats]))


# ------------------------------------------------------------------------------------------------ 4. graph == eager
def test_cached_graph_replay_equals_eager_launches(tiny):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 5
    x, ctx, _ = inputs(cfg, B, 4371)
    gen = torch.Generator().manual_seed(4372)
    lr_lat = (0.18215 * torch.randn((B, 4, HW, HW), generator=gen)).cuda()
    noise = torch.randn((n - 1, B, 4, HW, HW), generator=gen).cuda()
    sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    finals = {}
    for use_graph in (True, False):
        lat = x.cuda().clone()
        smp = mrisr.Sampler(tiny["unet"], sp, kind="resshift")
        smp.set_cache(2, 3)
        smp.run(lat, ctx.cuda(), lr_latents=lr_lat, step_noise=noise, use_graph=use_graph)
        torch.cuda.synchronize()
        finals[use_graph] = lat.cpu()
    assert torch.equal(finals[True], finals[False])
    assert not torch.equal(finals[True], x)


# ------------------------------------------------------------------------------------------------ 5. the sampler's state
def test_cache_state_on_one_sampler(tiny):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 6
    x, ctx, _ = inputs(cfg, B, 4381)
    _, sp = dd_scheduler(n)

    def run(smp, cache, rng=None):
        lat = x.cuda().clone()
        if cache is not None:
            smp.set_cache(*cache)
        for first, last in (rng or [(0, n)]):
            smp.set_range(first, last)
            smp.run(lat, ctx.cuda())
        torch.cuda.synchronize()
        return lat.cpu()

    fresh = lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim")  # noqa: E731
    one = fresh()
    seq = [(3, 1), (3, 1), (2, 2), (3, 2), (1, 1), (3, 1)]
    got = [run(one, c) for c in seq]
    for c, have in zip(seq, got):
        assert torch.equal(have, run(fresh(), c)), c  # changed on one sampler: the step graphs are captured again
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[5])  # two cached runs in a row; and after a detour
    assert torch.equal(got[4], run(fresh(), None))                      # back at interval 1: a sampler that never had a cache
    assert len({tuple(g.flatten()[:64].tolist()) for g in (got[0], got[2], got[3], got[4])}) == 4
    # a split run [0, 3) + [3, 6) at interval 3 is the whole run: each range starts with a full step, as steps 0 and 3 of the whole run are
    assert torch.equal(run(fresh(), (3, 1), [(0, 3), (3, 6)]), got[0])
    # ... and a range starting elsewhere starts full too (never an earlier run's cache): [0, 2) + [2, 6) is steps F S | F S S F
    ref_net = CachedUNet(tiny["p"], cfg, 3, 1)
    from oracle import sampler as osa
    so, _ = dd_scheduler(n)
    so.timesteps = so.timesteps[:2]
    head = osa.ddim_sample(ref_net, x, ctx, so)
    ref_net.reset()
    so2, _ = dd_scheduler(n)
    so2.timesteps = so2.timesteps[2:]
    tail = osa.ddim_sample(ref_net, head[-1], ctx, so2)
    assert ref_net.kinds == ["full", "shallow", "shallow", "full"]
    split = run(fresh(), (3, 1), [(0, 2), (2, 6)])
    assert rel(split, tail[-1]) < 1e-3 and maxrel(split, tail[-1]) < 1e-3


# ------------------------------------------------------------------------------------------------ 6. errors
def test_cache_errors_are_raised_before_any_launch(tiny):
    import mrisr
    from oracle import unet as ou
    L = mrisr._lib
    cfg, B, n = tiny["cfg"], 2, 3
    x, ctx, _ = inputs(cfg, B, 4391)
    _, sp = dd_scheduler(n)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    for bad in ((0, 1), (-1, 1), (2, 0), (2, 12), (2.0, 1), (2, 1.5), (True, 1)):
        with pytest.raises(ValueError):
            smp.set_cache(*bad)
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="f32")
    cnet.load_state_dict(ou.init_controlnet_params(cfg, seed=4392, perturb_norm=True))
    with_cn = mrisr.Sampler(tiny["unet"], sp, cnet, kind="ddim")
    with pytest.raises(ValueError, match="ControlNet"):
        with_cn.set_cache(2, 1)
    with_cn.set_cache(1, 1)  # interval 1 is no cache
    # the C ABI refuses the same by itself
    for h, interval, depth, what in ((smp._h, 0, 1, "interval"), (smp._h, 2, 0, "depth"), (smp._h, 2, 12, "depth"), (with_cn._h, 2, 1, "ControlNet")):
        with pytest.raises(RuntimeError, match=what):
            L.check(L.lib().mrisr_sampler_set_cache(h, interval, depth))
    lat = x.cuda().clone()
    smp.run(lat, ctx.cuda())  # none of the refused calls left a cache behind: the plain run
    ref = x.cuda().clone()
    mrisr.Sampler(tiny["unet"], sp, kind="ddim").run(ref, ctx.cuda())
    torch.cuda.synchronize()
    assert torch.equal(lat, ref)

    # forward_cached: a cache of the wrong shape, dtype or layout
    net, d = tiny["unet"], 5
    b, c, h, w = net.cache_shape(d, B, HW, HW)
    assert (b, c, h, w) == (B, 256, 8, 8)
    t = torch.tensor(500).cuda()
    good = torch.zeros((b, h, w, c), device="cuda")
    bad_caches = [torch.zeros((b, h, w, c // 2), device="cuda"),            # shape
                  torch.zeros((b + 1, h, w, c), device="cuda"),
                  torch.zeros((b, c, h, w), device="cuda"),                  # NCHW
                  torch.zeros((b, h, w, c), device="cuda", dtype=torch.bfloat16),  # not the compute dtype
                  torch.zeros((b, h, w, 2 * c), device="cuda")[..., ::2],   # not contiguous
                  torch.zeros((b, h, w, c))]                                 # not on the device
    for cache in bad_caches:
        for shallow in (False, True):
            with pytest.raises(ValueError):
                net.forward_cached(x.cuda(), t, ctx.cuda(), cache, d, shallow)
    for depth in (0, 12):
        with pytest.raises(RuntimeError, match="depth"):
            net.forward_cached(x.cuda(), t, ctx.cuda(), good, depth, False)
    torch.cuda.synchronize()
    assert not bool(good.any())  # nothing was written

    def raw(cache_t, depth=d, shallow=0):
        out = torch.full((B, 4, HW, HW), float("nan"), device="cuda")
        xs, cs = x.cuda(), ctx.cuda()
        t_s, t_t, t_e, t_o = L.as_tensor(xs), L.as_tensor(t), L.as_tensor(cs), L.as_tensor(out)
        rc = L.lib().mrisr_unet_forward_cached(net._h, C.byref(t_s), C.byref(t_t), C.byref(t_e), None, 0, depth, shallow, C.byref(cache_t),
                                               C.byref(t_o), L.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    nhwc = lambda tt, shape=(b, c, h, w): L.as_tensor(tt, layout=L.MRISR_NHWC, shape=shape)  # noqa: E731
    bf = torch.zeros((b, h, w, c), device="cuda", dtype=torch.bfloat16)
    for cache_t in (L.as_tensor(good, shape=(b, c, h, w)),      # layout NCHW
                    nhwc(bf),                                    # dtype
                    nhwc(good, (b, c // 2, h, w)),               # shape
                    nhwc(good, (b, c, h, 2 * w)),
                    L.Tensor()):                                 # no data at all
        rc, out = raw(cache_t)
        assert rc != 0 and "feature cache" in L.lib().mrisr_last_error().decode()
        assert bool(torch.isnan(out).all())
    rc, out = raw(nhwc(good), depth=12)
    assert rc != 0 and "depth" in L.lib().mrisr_last_error().decode() and bool(torch.isnan(out).all())
    assert not bool(good.any())
    rc, out = raw(nhwc(good))  # and the well-formed call runs
    assert rc == 0 and bool(torch.isfinite(out).all()) and bool(good.any())


# ------------------------------------------------------------------------------------------------ 7. log_validation
class _StubVAE:
    class config:
        scaling_factor = 0.18215

    def encode(self, x):
        z = torch.nn.functional.avg_pool2d(x[:, :1], 8).repeat(1, 4, 1, 1)
        return type("E", (), {"latent_dist": type("D", (), {"sample": staticmethod(lambda: z)})})

    def decode(self, z):
        return type("O", (), {"sample": torch.nn.functional.interpolate(z.mean(1, keepdim=True), scale_factor=8.0, mode="nearest")})


def test_log_validation_with_cache_equals_the_pipeline_by_hand(tiny):
    import mrisr
    cfg, n = tiny["cfg"], 4
    gen = torch.Generator().manual_seed(4401)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(128, 128), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    ctx = torch.randn((1, 77, cfg.cross_attention_dim), generator=gen)
    vae, acc = _StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(4402)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(tiny["unet"], None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx.cuda(),
                                               num_inference_steps=n, **kw))

    got = panel(cache_interval=2, cache_depth=1)
    torch.manual_seed(4402)
    sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    lr_d = lr.cuda()
    anchor = (vae.encode(lr_d.expand(-1, 3, -1, -1)).latent_dist.sample() * vae.config.scaling_factor).float()
    sched.set_timesteps(n, device="cuda")
    lat = mrisr.get_res_shifting_latents(anchor, anchor, sched.timesteps[0], sched).contiguous()
    noise = torch.stack([torch.randn_like(lat) for _ in range(n - 1)])
    smp = mrisr.Sampler(tiny["unet"], sched, None, kind="resshift")
    smp.set_cache(2, 1)
    smp.run(lat, ctx.cuda(), lr_latents=anchor, step_noise=noise)
    W = got.shape[1] // 3
    assert np.array_equal(got[:, W:2 * W], mrisr.decode_to_vis(lat, vae))
    assert np.array_equal(got[:, :W], mrisr.decode_to_vis(lr_d, vae, is_latent=False))
    # the defaults change nothing
    plain = panel()
    assert np.array_equal(plain, panel(cache_interval=1, cache_depth=1))
    assert not np.array_equal(plain[:, W:2 * W], got[:, W:2 * W])
    with pytest.raises(ValueError):
        panel(cache_interval=2, cache_depth=12)


# ------------------------------------------------------------------------------------------------ 8. SD-1.5 width (last: the expensive one)
@pytest.fixture(scope="module")
def wide():
    """Full-width parameters and ONE reference trajectory shared by the f32 and the bf16 case: B = 2, 32 x 32, the first two steps of the
    50-step DDIM schedule at interval 2 / depth 1 (one full and one shallow oracle forward)."""
    from oracle import sampler as osa
    from oracle import schedulers as osch
    from oracle import unet as ou
    cfg = ou.SD15
    p = ou.init_unet_params(cfg, seed=1101, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=1103))
    x, ctx, _ = inputs(cfg, 2, 4411, hw=32)
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(50)
    so.timesteps = so.timesteps[:2]
    ref_net = CachedUNet(p, cfg, 2, 1)
    traj = osa.ddim_sample(ref_net, x, ctx, so)
    assert ref_net.kinds == ["full", "shallow"]
    yield dict(cfg=cfg, p=p, x=x, ctx=ctx, so=so, traj=traj)
    gc.collect()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_zz_cached_ddim_sd15_width(wide, dt):
    """The only place the level-0 fused kernels (the fused feed-forward, the fused cross-attention middle, halo convs over a concat) run
    as a shallow step.  Both states of the run against the reference; for bf16 also the prediction each step consumed."""
    import mrisr
    net = mrisr.UNet2DConditionModel(mrisr.UNetConfig(), compute_dtype=dt, lora_rank=4, lora_alpha=4, lora_fused=True, flash_attention=True)
    net.load_state_dict(wide["p"])
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(50)
    so, traj = wide["so"], wide["traj"]
    smp = mrisr.Sampler(net, sp, kind="ddim")
    smp.set_cache(2, 1)
    tol = 1e-3 if dt == "f32" else 5e-2
    states = [wide["x"]]
    for k in (1, 2):
        lat = wide["x"].cuda().clone()
        smp.set_range(0, k)
        smp.run(lat, wide["ctx"].cuda())
        torch.cuda.synchronize()
        states.append(lat.cpu())
    figures = []
    for k in (1, 2):
        t = int(so.timesteps[k - 1])
        cx, ce = so.ddim_coeffs(t)
        e_dev = (states[k].double() - cx * states[k - 1].double()) / ce  # the prediction step k consumed
        e_ref = (traj[k].double() - cx * traj[k - 1].double()) / ce
        figures.append((rel(states[k], traj[k]), maxrel(states[k], traj[k]), rel(e_dev, e_ref)))
        print(f"SD-1.5 width [{dt}] cached DDIM step {k} ({'full' if k == 1 else 'shallow'}): state rel {figures[-1][0]:.3e} "
              f"maxrel {figures[-1][1]:.3e}, eps rel {figures[-1][2]:.3e}")
    del smp, net
    gc.collect()
    torch.cuda.empty_cache()
    for r, m, re in figures:
        assert r < tol and re < tol and (dt == "bf16" or m < tol), figures
