"""GPU: tiled sampling in the graph sampler - the gather and the blend kernels alone (bit-equal to slicing / against the float64
blend on the same f32 tables), tiled trajectories against the wrapped CPU oracle (tests/tiles_ref.py, itself checked by
test_tiles_cpu.py), graph == eager, "off means off", no stale graph or table between runs on one sampler, bf16, ``log_validation``
plumbing and the errors.  f32 engine unless stated.

Tolerances: the blend alone 1e-6 (a canvas element is at most 9 products of two f32 weights and a value, summed in f32);
trajectories 1e-3 relative L2 and max-relative (the f32 tolerance of every sampler test here); bf16 5e-2 (the unguided factor of
test_gpu_guidance.py::test_guided_ddim_step_bf16's bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

import multistep_ref as mref
import tiles_ref as tr
from guidance_ref import GuidedUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BF16_BOUND = 5e-2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def maxrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
def _ints(v):
    return (C.c_int * len(v))(*v)


def op_gather(x, oy, ox, th, tw):
    import mrisr
    L = mrisr._lib
    xt = torch.full((x.shape[0] * len(oy) * len(ox), x.shape[1], th, tw), float("nan"), device=x.device)
    t_x, t_xt = L.as_tensor(x), L.as_tensor(xt)
    L.check(L.lib().mrisr_op_tile_gather(C.byref(t_x), C.byref(t_xt), _ints(oy), len(oy), _ints(ox), len(ox), L.stream_ptr()))
    return xt


def op_blend(et, oy, ox, nwy, nwx, H, W):
    """nwy / nwx: f32 CPU tables [k][tile]."""
    import mrisr
    L = mrisr._lib
    out = torch.full((et.shape[0] // (len(oy) * len(ox)), et.shape[1], H, W), float("nan"), device=et.device)
    nwy, nwx = nwy.contiguous(), nwx.contiguous()
    t_e, t_o = L.as_tensor(et), L.as_tensor(out)
    L.check(L.lib().mrisr_op_tile_blend(C.byref(t_e), C.byref(t_o), _ints(oy), len(oy), _ints(ox), len(ox),
                                        C.c_void_p(nwy.data_ptr()), C.c_void_p(nwx.data_ptr()), L.stream_ptr()))
    return out


def tables(H, W, tile, overlap, window):
    import mrisr
    oy, nwy = mrisr.tile_tables(H, tile, overlap, window)
    ox, nwx = mrisr.tile_tables(W, tile, overlap, window)
    return oy, ox, nwy, nwx, min(tile, H), min(tile, W)


KERNEL_SHAPES = [  # B, C, H, W, tile, overlap
    (1, 4, 24, 32, 16, 8),   # non-square, 2 x 3 tiles
    (3, 4, 40, 40, 16, 0),   # pulled-back last tile on both axes
    (2, 1, 12, 8, 4, 2),     # d = 2: the scalar path
    (2, 4, 64, 64, 32, 8),
    (2, 4, 16, 16, 16, 0),   # T = 1: the blend returns its input bit for bit
]


@pytest.mark.parametrize("window", ["gaussian", "uniform"])
@pytest.mark.parametrize("B,Cc,H,W,tile,overlap", KERNEL_SHAPES)
def test_gather_and_blend_kernels(B, Cc, H, W, tile, overlap, window):
    gen = torch.Generator().manual_seed(6000 + H * 100 + W)
    oy, ox, nwy, nwx, th, tw = tables(H, W, tile, overlap, window)
    T = len(oy) * len(ox)
    x = torch.randn((B, Cc, H, W), generator=gen).cuda()
    xt = op_gather(x, oy, ox, th, tw)
    assert torch.equal(xt, tr.gather(x, oy, ox, th, tw))  # a copy: bit-equal to slicing
    et = torch.randn((B * T, Cc, th, tw), generator=gen).cuda()  # unrelated tile predictions: the sum itself is under test
    out = op_blend(et, oy, ox, nwy, nwx, H, W)
    ref = tr.blend(et.cpu(), oy, ox, nwy, nwx, H, W)
    m = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
    r = rel(out, ref)
    print(f"tile blend B={B} C={Cc} {H}x{W} tile={tile} overlap={overlap} {window} (T={T}): max-abs/max|ref| {m:.3e} rel-l2 {r:.3e}")
    assert m <= 1e-6 and r <= 1e-6, (m, r)
    assert torch.equal(op_blend(et, oy, ox, nwy, nwx, H, W), out)  # no atomics, a fixed order: two launches, the same bits
    if T == 1:
        assert torch.equal(out, et)
    # and the round trip: blend(gather(x)) is x up to the rounding of the weights
    back = op_blend(xt, oy, ox, nwy, nwx, H, W)
    assert maxrel(back, x) <= 1e-6


def test_blend_of_constant_tiles_is_their_convex_combination_and_samples_are_isolated():
    B, Cc, H, W, tile, overlap = 3, 2, 24, 32, 16, 8
    oy, ox, nwy, nwx, th, tw = tables(H, W, tile, overlap, "gaussian")
    T = len(oy) * len(ox)
    consts = torch.arange(1, B * T * Cc + 1, dtype=torch.float32).reshape(B * T, Cc, 1, 1) * 0.37
    et = consts.expand(-1, -1, th, tw).contiguous().cuda()
    out = op_blend(et, oy, ox, nwy, nwx, H, W).cpu().double()
    ref = torch.zeros((B, Cc, H, W), dtype=torch.float64)
    lo = torch.full((B, Cc, H, W), float("inf"), dtype=torch.float64)
    hi = -lo.clone()
    for iy, y in enumerate(oy):      # written out here, not through tiles_ref: a wrong tile index or a swapped axis shows
        for ix, xx in enumerate(ox):
            for b in range(B):
                c = consts[b * T + iy * len(ox) + ix].double()
                wgt = nwy[iy].double()[:, None] * nwx[ix].double()[None, :]
                ref[b, :, y:y + th, xx:xx + tw] += wgt * c
                lo[b, :, y:y + th, xx:xx + tw] = torch.minimum(lo[b, :, y:y + th, xx:xx + tw], c.expand(-1, th, tw))
                hi[b, :, y:y + th, xx:xx + tw] = torch.maximum(hi[b, :, y:y + th, xx:xx + tw], c.expand(-1, th, tw))
    assert float((out - ref).abs().max() / ref.abs().max()) <= 1e-6
    assert bool((out >= lo * (1 - 1e-6)).all()) and bool((out <= hi * (1 + 1e-6)).all())  # between the covering tiles' constants
    # replacing sample 1's tiles leaves the other samples' canvas bits alone
    gen = torch.Generator().manual_seed(6101)
    et = torch.randn((B * T, Cc, th, tw), generator=gen).cuda()
    base = op_blend(et, oy, ox, nwy, nwx, H, W)
    other = et.clone()
    other[T:2 * T] = 5.0 * torch.randn((T, Cc, th, tw), generator=gen).cuda()
    out = op_blend(other, oy, ox, nwy, nwx, H, W)
    assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2]) and not torch.equal(out[1], base[1])


# ------------------------------------------------------------------------------------------------ models
@pytest.fixture(scope="module")
def tiny():
    """TINY UNet (+ rank-4 LoRA) and ControlNet: oracle callables and one f32 device model of each."""
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=6201, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=6203))
    cp = ou.init_controlnet_params(cfg, seed=6202, perturb_norm=True)
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    unet.load_state_dict(p)
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="f32")
    cnet.load_state_dict(cp)
    return dict(cfg=cfg, p=p, cp=cp, unet=unet, cnet=cnet, o_unet=ou.OracleUNet(p, cfg), o_cnet=ou.OracleControlNet(cp, cfg))


H0, W0, TILE, OVER = 24, 32, 16, 8  # the canvas of the trajectory tests: 2 x 3 tiles


def contexts(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, 77, cfg.cross_attention_dim), generator=g), torch.randn((B, 77, cfg.cross_attention_dim), generator=g)


def ddim_schedulers(n):
    import mrisr
    from oracle import schedulers as osch
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    return so, sp


def tiled_sampler(unet, sp, cnet=None, kind="ddim", tile=TILE, overlap=OVER, window="gaussian"):
    import mrisr
    smp = mrisr.Sampler(unet, sp, cnet, kind=kind)
    smp.set_tiles(tile, overlap, window)
    return smp


def check_states(tag, make_sampler, x0, oracle_traj, n, run_kw):
    smp = make_sampler()
    for k in range(1, n + 1):
        lat = x0.clone().contiguous()
        smp.set_range(0, k)
        smp.run(lat, **run_kw)
        torch.cuda.synchronize()
        r, m = rel(lat, oracle_traj[k]), maxrel(lat, oracle_traj[k])
        print(f"{tag}: state {k}/{n} rel {r:.3e} maxrel {m:.3e}")
        assert r < 1e-3 and m < 1e-3, (tag, k, r, m)


def check_final(tag, make_sampler, x0, ref, run_kw):
    lat = x0.clone().contiguous()
    make_sampler().run(lat, **run_kw)
    torch.cuda.synchronize()
    r, m = rel(lat, ref), maxrel(lat, ref)
    print(f"{tag}: final state rel {r:.3e} maxrel {m:.3e}")
    assert r < 1e-3 and m < 1e-3, (tag, r, m)


# ------------------------------------------------------------------------------------------------ 2. trajectories
def test_tiled_ddim_trajectory_with_lora(tiny):
    from oracle import sampler as osa
    cfg, B, n = tiny["cfg"], 2, 5
    _, ctx = contexts(cfg, B, 6301)
    x = torch.randn((B, 4, H0, W0), generator=torch.Generator().manual_seed(6302))
    so, sp = ddim_schedulers(n)
    wrapped = tr.TiledUNet(tiny["o_unet"], H0, W0, TILE, OVER)
    assert wrapped.T == 6
    traj = osa.ddim_sample(wrapped, x, ctx, so)
    check_states("tiled ddim+lora", lambda: tiled_sampler(tiny["unet"], sp), x.cuda(), traj, n, dict(encoder_hidden_states=ctx.cuda()))


def test_tiled_res_srdiff_trajectory_with_controlnet_anchor_and_noise(tiny):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n = tiny["cfg"], 2, 5
    _, ctx = contexts(cfg, B, 6311)
    gen = torch.Generator().manual_seed(6312)
    lr_lat = 0.18215 * torch.randn((B, 4, H0, W0), generator=gen)
    cond = torch.randn((B, 3, 8 * H0, 8 * W0), generator=gen)
    init_noise = torch.randn(lr_lat.shape, generator=gen)
    step_noise = torch.stack([torch.randn(lr_lat.shape, generator=gen) for _ in range(n - 1)])
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    traj = osa.res_srdiff_sample(tr.TiledUNet(tiny["o_unet"], H0, W0, TILE, OVER), tr.TiledControlNet(tiny["o_cnet"], H0, W0, TILE, OVER),
                                 lr_lat, ctx, cond, so.timesteps, so.alphas_cumprod, init_noise, list(step_noise))
    sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, init_noise.cuda())
    assert rel(x0, traj[0]) < 1e-5
    kw = dict(encoder_hidden_states=ctx.cuda(), lr_latents=lr_lat.cuda(), step_noise=step_noise.cuda(), controlnet_cond=cond.cuda())
    check_final("tiled res-srdiff+controlnet", lambda: tiled_sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift"), x0, traj[-1], kw)


def test_tiled_ddim_trajectory_with_adapter_features(tiny):
    from oracle import adapter as oad
    from oracle import sampler as osa
    cfg, B, n = tiny["cfg"], 2, 5
    gen = torch.Generator().manual_seed(6321)
    image = torch.randn((B, 3, 8 * H0, 8 * W0), generator=gen)  # a 192 x 256 px condition: the adapter runs ONCE on all of it
    feats = oad.adapter_forward(oad.init_adapter_params(oad.ADAPTER_TINY, seed=6322), oad.ADAPTER_TINY, image)
    assert [tuple(f.shape[2:]) for f in feats] == [(24, 32), (12, 16), (6, 8), (3, 4)]
    _, ctx = contexts(cfg, B, 6323)
    x = torch.randn((B, 4, H0, W0), generator=gen)
    so, sp = ddim_schedulers(n)
    traj = osa.ddim_sample(tr.TiledUNet(tiny["o_unet"], H0, W0, TILE, OVER), x, ctx, so, intrablock=[f.clone() for f in feats])
    kw = dict(encoder_hidden_states=ctx.cuda(), adapter_features=[f.cuda() for f in feats])
    check_final("tiled ddim+adapter", lambda: tiled_sampler(tiny["unet"], sp), x.cuda(), traj[-1], kw)


def test_tiled_guided_ddim_trajectory(tiny):
    from oracle import sampler as osa
    cfg, B, n, g, phi = tiny["cfg"], 2, 5, 3.0, 0.7
    ctx_u, ctx_c = contexts(cfg, B, 6331)
    x = torch.randn((B, 4, H0, W0), generator=torch.Generator().manual_seed(6332))
    so, sp = ddim_schedulers(n)
    wrapped = GuidedUNet(tr.TiledUNet(tiny["o_unet"], H0, W0, TILE, OVER), ctx_u.expand(B, -1, -1), ctx_c, g, phi)
    traj = osa.ddim_sample(wrapped, x, None, so)
    kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi)
    check_final("tiled guided ddim", lambda: tiled_sampler(tiny["unet"], sp), x.cuda(), traj[-1], kw)


def test_tiled_unipc_trajectory_with_lr_anchor(tiny):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 5
    _, ctx = contexts(cfg, B, 6341)
    gen = torch.Generator().manual_seed(6342)
    lr_lat = 0.18215 * torch.randn((B, 4, H0, W0), generator=gen)
    sp = mrisr.UniPCMultistepScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, torch.randn(lr_lat.shape, generator=gen).cuda())
    ref = mref.multistep_sample("unipc", tr.TiledUNet(tiny["o_unet"], H0, W0, TILE, OVER), x0.cpu(), ctx, sp.timesteps, sp.alphas_cumprod,
                                lr_latents=lr_lat)
    kw = dict(encoder_hidden_states=ctx.cuda(), lr_latents=lr_lat.cuda())
    check_final("tiled unipc+anchor", lambda: tiled_sampler(tiny["unet"], sp, kind="unipc"), x0, ref[-1], kw)


def test_tiled_uniform_window_without_overlap(tiny):
    """Canvas 32 x 32, tile 16, overlap 0: four disjoint tiles, every weight 1 - no blending, only the batch plumbing."""
    import mrisr
    from oracle import sampler as osa
    cfg, B, n = tiny["cfg"], 2, 4
    _, ctx = contexts(cfg, B, 6351)
    x = torch.randn((B, 4, 32, 32), generator=torch.Generator().manual_seed(6352))
    so, sp = ddim_schedulers(n)
    wrapped = tr.TiledUNet(tiny["o_unet"], 32, 32, 16, 0, "uniform")
    assert wrapped.T == 4 and bool((wrapped.nwy == 1).all()) and bool((wrapped.nwx == 1).all())
    assert bool((mrisr.tile_tables(32, 16, 0, "uniform")[1] == 1).all())
    traj = osa.ddim_sample(wrapped, x, ctx, so)
    check_final("tiled ddim uniform", lambda: tiled_sampler(tiny["unet"], sp, overlap=0, window="uniform"), x.cuda(), traj[-1],
                dict(encoder_hidden_states=ctx.cuda()))


# ------------------------------------------------------------------------------------------------ 3. plumbing
def resshift_setup(tiny, h=H0, w=W0, B=2, n=4, seed=6401):
    import mrisr
    gen = torch.Generator().manual_seed(seed)
    lr_lat = (0.18215 * torch.randn((B, 4, h, w), generator=gen)).cuda()
    sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    x0 = mrisr.get_res_shifting_latents(lr_lat, lr_lat, sp.timesteps[0], sp, torch.randn(lr_lat.shape, generator=gen).cuda())
    _, ctx = contexts(tiny["cfg"], B, seed + 1)
    kw = dict(encoder_hidden_states=ctx.cuda(), lr_latents=lr_lat,
              step_noise=torch.stack([torch.randn(lr_lat.shape, generator=gen) for _ in range(n - 1)]).cuda(),
              controlnet_cond=torch.randn((B, 3, 8 * h, 8 * w), generator=gen).cuda())
    return sp, x0, kw


def run_copy(smp, x0, **kw):
    lat = x0.clone().contiguous()
    smp.run(lat, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


def test_tiled_graph_replay_equals_eager_launches(tiny):
    sp, x0, kw = resshift_setup(tiny)
    finals = {g: run_copy(tiled_sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift"), x0, use_graph=g, **kw) for g in (True, False)}
    assert torch.equal(finals[True], finals[False])
    assert not torch.equal(finals[True], x0.cpu())


def test_tiles_off_means_off(tiny):
    import mrisr
    sp, x0, kw = resshift_setup(tiny, h=16, w=16)
    fresh = lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift")  # noqa: E731
    plain = run_copy(fresh(), x0, **kw)
    never = fresh()
    never.set_tiles(None)
    assert torch.equal(run_copy(never, x0, **kw), plain)
    covering = fresh()
    covering.set_tiles(16, 8)  # one tile: T == 1
    assert covering.tile_rows(2, 16, 16) == 2
    assert torch.equal(run_copy(covering, x0, **kw), plain)
    bigger = fresh()
    bigger.set_tiles((32, 16), 0, "uniform")
    assert torch.equal(run_copy(bigger, x0, **kw), plain)
    toggled = fresh()
    toggled.set_tiles(8, 0)
    tiled = run_copy(toggled, x0, **kw)
    assert not torch.equal(tiled, plain)
    toggled.set_tiles(None)
    assert torch.equal(run_copy(toggled, x0, **kw), plain)


def test_tiles_do_not_go_stale_on_one_sampler(tiny):
    """Tiled at one canvas, then at another canvas size (other grid, other tables, other buffers), then the first again, then another
    window: each equals a fresh sampler's run."""
    sp, xa, kwa = resshift_setup(tiny, h=24, w=32, seed=6411)
    _, xb, kwb = resshift_setup(tiny, h=32, w=16, seed=6413)
    one = tiled_sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift")
    seq = [(xa, kwa, "gaussian"), (xb, kwb, "gaussian"), (xa, kwa, "gaussian"), (xa, kwa, "uniform")]
    got = []
    for x0, kw, window in seq:
        one.set_tiles(TILE, OVER, window)
        got.append(run_copy(one, x0, **kw))
    for (x0, kw, window), have in zip(seq, got):
        assert torch.equal(have, run_copy(tiled_sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift", window=window), x0, **kw)), window
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[3])


def test_tile_rows(tiny):
    import mrisr
    _, sp = ddim_schedulers(3)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    assert smp.tile_rows(3, 64, 64) == 3
    smp.set_tiles(32, 0)
    assert smp.tile_rows(8, 64, 64) == 32 and smp.tile_rows(8, 32, 32) == 8 and smp.tile_rows(2, 64, 32) == 4
    smp.set_tiles(32, 8)
    assert smp.tile_rows(8, 64, 64) == 72 and smp.tile_rows(1, 64, 64, guided=True) == 18
    smp.set_tiles(32, 16)
    assert smp.tile_rows(8, 64, 64) == 72 and smp.tile_rows(1, 80, 48) == 8
    smp.set_tiles((16, 32), (8, 0))
    assert smp.tile_rows(2, 24, 32) == 4
    with pytest.raises(ValueError):
        smp.tile_rows(1, 20, 32)
    smp.set_tiles(None)
    assert smp.tile_rows(5, 20, 36) == 5


# ------------------------------------------------------------------------------------------------ 4. bf16
def test_tiled_ddim_bf16_against_the_f32_engine(tiny):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 3
    _, ctx = contexts(cfg, B, 6501)
    x = torch.randn((B, 4, H0, W0), generator=torch.Generator().manual_seed(6502)).cuda()
    _, sp = ddim_schedulers(n)
    ref = run_copy(tiled_sampler(tiny["unet"], sp), x, encoder_hidden_states=ctx.cuda())
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    got = run_copy(tiled_sampler(net, sp), x, encoder_hidden_states=ctx.cuda())
    r = rel(got, ref)
    print(f"tiled 3-step DDIM, bf16 engine vs f32 engine: rel {r:.3e} (bound {BF16_BOUND})")
    assert r < BF16_BOUND, r


# ------------------------------------------------------------------------------------------------ 5. log_validation
class _StubVAE:
    class config:
        scaling_factor = 0.18215

    def encode(self, x):
        z = torch.nn.functional.avg_pool2d(x[:, :1], 8).repeat(1, 4, 1, 1)
        return type("E", (), {"latent_dist": type("D", (), {"sample": staticmethod(lambda: z)})})

    def decode(self, z):
        return type("O", (), {"sample": torch.nn.functional.interpolate(z.mean(1, keepdim=True), scale_factor=8.0, mode="nearest")})


def test_log_validation_with_tiles_equals_the_pipeline_by_hand(tiny):
    import mrisr
    cfg, n = tiny["cfg"], 3
    gen = torch.Generator().manual_seed(6601)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(256, 256), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    _, ctx = contexts(cfg, 1, 6602)
    vae, acc = _StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(6603)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(tiny["unet"], None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx.cuda(),
                                               num_inference_steps=n, **kw))

    got = panel(tile=16, tile_overlap=8, tile_window="gaussian")
    torch.manual_seed(6603)  # by hand: the same draws from the same global stream, in the same order
    sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    lr_d = lr.cuda()
    anchor = (vae.encode(lr_d.expand(-1, 3, -1, -1)).latent_dist.sample() * vae.config.scaling_factor).float()
    sched.set_timesteps(n, device="cuda")
    lat = mrisr.get_res_shifting_latents(anchor, anchor, sched.timesteps[0], sched).contiguous()
    noise = torch.stack([torch.randn_like(lat) for _ in range(n - 1)])
    smp = mrisr.Sampler(tiny["unet"], sched, None, kind="resshift")
    smp.set_tiles(16, 8, "gaussian")
    assert smp.tile_rows(1, 32, 32) == 9
    smp.run(lat, ctx.cuda(), lr_latents=anchor, step_noise=noise)
    Wp = got.shape[1] // 3
    assert np.array_equal(got[:, Wp:2 * Wp], mrisr.decode_to_vis(lat, vae))
    assert np.array_equal(got[:, :Wp], mrisr.decode_to_vis(lr_d, vae, is_latent=False))
    plain = panel()  # the arguments do something, and their defaults nothing
    assert not np.array_equal(plain[:, Wp:2 * Wp], got[:, Wp:2 * Wp])
    assert np.array_equal(plain, panel(tile=None, tile_overlap=0, tile_window="gaussian"))


# ------------------------------------------------------------------------------------------------ 6. errors
def test_tile_errors_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    B, n = 2, 3
    gen = torch.Generator().manual_seed(6701)
    _, ctx = contexts(tiny["cfg"], B, 6702)
    _, sp = ddim_schedulers(n)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    for kw in (dict(tile=4), dict(tile=12), dict(tile=(16, 20)), dict(tile=16, overlap=-8), dict(tile=16, overlap=16),
               dict(tile=16, overlap=4), dict(tile=16, overlap=8, window="hann"), dict(tile=16.0)):
        with pytest.raises(ValueError):
            smp.set_tiles(**kw)
    assert smp.tiles is None
    # tiles + cache, in both orders (Python and the C ABI each refuse)
    smp.set_cache(2, 1)
    with pytest.raises(ValueError, match="cache"):
        smp.set_tiles(16, 8)
    with pytest.raises(RuntimeError, match="cache"):
        L.check(L.lib().mrisr_sampler_set_tiles(smp._h, 16, 16, 8, 8, 1))
    smp.set_cache(1, 1)
    smp.set_tiles(16, 8)
    with pytest.raises(ValueError, match="tiles"):
        smp.set_cache(2, 1)
    with pytest.raises(RuntimeError, match="tiles"):
        L.check(L.lib().mrisr_sampler_set_cache(smp._h, 2, 1))
    for args in ((12, 16, 0, 0, 1), (16, 16, 4, 8, 1), (16, 16, 8, 16, 1), (16, 16, 8, 8, 2), (16, 4, 0, 0, 1)):
        with pytest.raises(RuntimeError):
            L.check(L.lib().mrisr_sampler_set_tiles(smp._h, *args))

    x = torch.randn((B, 4, H0, W0), generator=gen).cuda()
    lat = x.clone()
    odd = torch.randn((B, 4, 20, 32), generator=gen).cuda()  # a canvas not divisible by d = 8
    with pytest.raises(ValueError, match="multiples of 8"):
        smp.run(odd.clone(), ctx.cuda())
    for feats in ([torch.zeros((B, 64, 24, 16))], [torch.zeros((B, 64, 16, 32))], [torch.zeros((B, 64, 8, 8))],
                  [torch.zeros((B, 64, 24, 32)), torch.zeros((B, 128, 12, 12))], [torch.zeros((1, 64, 24, 32))]):
        with pytest.raises(ValueError, match="adapter features"):  # shapes that do not fit the canvas
            smp.run(lat, ctx.cuda(), adapter_features=[f.cuda() for f in feats])
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran

    # the C ABI validates the tile batch itself: T = 6 here, so 12 rows at 16 x 16
    def run_c(ehs, latents=lat, feats=(), cond=None, sampler=smp):
        t_lat, t_e = L.as_tensor(latents), L.as_tensor(ehs)
        t_c = L.as_tensor(cond) if cond is not None else None
        f_arr = L.tensor_array([L.as_tensor(f) for f in feats])
        L.check(L.lib().mrisr_sampler_run(sampler._h, C.byref(t_lat), None, None, C.byref(t_e), C.byref(t_c) if t_c else None,
                                          f_arr if feats else None, len(feats), 1, L.stream_ptr()))

    ehs_t = ctx.cuda().repeat_interleave(6, dim=0).contiguous()
    with pytest.raises(RuntimeError, match="encoder_hidden_states"):
        run_c(ctx.cuda().contiguous())                                        # [B] rows where B * T are needed
    with pytest.raises(RuntimeError, match="encoder_hidden_states"):
        run_c(ehs_t[:11].contiguous())
    with pytest.raises(RuntimeError, match="adapter features"):
        run_c(ehs_t, feats=[torch.zeros((B, 64, 16, 16)).cuda()])             # a [B] feature in a tiled run
    with pytest.raises(RuntimeError, match="adapter features"):
        run_c(ehs_t, feats=[torch.zeros((12, 64, 24, 32)).cuda()])            # canvas geometry where tile geometry is needed
    with pytest.raises(RuntimeError, match="multiples"):
        run_c(ehs_t, latents=odd)
    csmp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    csmp.set_tiles(16, 8)
    with pytest.raises(RuntimeError, match="controlnet_cond"):
        run_c(ehs_t, cond=torch.zeros((B, 3, 8 * H0, 8 * W0)).cuda(), sampler=csmp)   # the canvas image, uncropped
    with pytest.raises(RuntimeError, match="controlnet_cond"):
        run_c(ehs_t, cond=torch.zeros((12, 3, 64, 128)).cuda(), sampler=csmp)
    # the single-op entries: shapes, origins out of range or not increasing, null tables
    oy, ox, nwy, nwx, th, tw = tables(H0, W0, TILE, OVER, "gaussian")
    with pytest.raises(RuntimeError):
        op_gather(x, oy, [0, 8, 24], th, tw)          # past the right edge
    with pytest.raises(RuntimeError):
        op_gather(x, oy, [0, 16, 8], th, tw)          # not increasing
    with pytest.raises(RuntimeError):
        op_gather(x, [0], ox, th, tw)                 # rows 16 .. 23 uncovered
    with pytest.raises(RuntimeError):
        op_gather(x, oy, ox, th, tw + 4)              # the tile does not match the grid
    with pytest.raises(RuntimeError):
        op_blend(torch.zeros((11, 4, th, tw)).cuda(), oy, ox, nwy, nwx, H0, W0)   # row count
    with pytest.raises(RuntimeError):
        t_x, t_t = L.as_tensor(x), L.as_tensor(torch.zeros((12, 4, th, tw)).cuda())
        L.check(L.lib().mrisr_op_tile_blend(C.byref(t_t), C.byref(t_x), _ints(oy), len(oy), _ints(ox), len(ox), None, None, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(lat, x)
    run_c(ehs_t)  # and the well-formed call runs
    torch.cuda.synchronize()
    assert not torch.equal(lat, x) and bool(torch.isfinite(lat).all())
