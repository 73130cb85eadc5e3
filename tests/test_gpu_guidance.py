"""GPU: classifier-free guidance in the graph sampler - the fused guided step alone against the formulae in float64, guided
trajectories of all three step kinds against the wrapped CPU oracle (tests/guidance_ref.py, itself checked by
test_guidance_cpu.py), graph == eager, "off means off", no stale state between runs on one sampler, bf16, SD-1.5 width,
``log_validation`` / ``fit`` plumbing and the errors.  f32 engine unless stated.

Tolerances: the kernel alone 1e-5 (a handful of f32 operations per element and two tree sums over <= 16 Ki f32 terms, each a few
1e-7); trajectories 1e-3 relative L2 and max-relative (the f32 tolerance of every sampler test here); bf16 3 x 5e-2 (guidance
computes g eps_c - (g-1) eps_u, which can amplify the single-forward bf16 bound by 2g-1 = 3 at g = 2)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from guidance_ref import GuidedControlNet, GuidedUNet, guided_eps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DDIM, RESSHIFT, DDPM = 0, 1, 2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def maxrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def coef_row(kind, a_t=0.37, a_p=0.52):
    """One realistic coefficient row per step kind, as mrisr_sampler_create builds them (rounded to f32: kernel and reference
    read the same numbers)."""
    if kind == DDIM:
        row = [np.sqrt(a_p / a_t), np.sqrt(1 - a_p) - np.sqrt(a_p * (1 - a_t) / a_t)]
    elif kind == RESSHIFT:
        row = [np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))]
    else:
        al = a_t / a_p
        row = [1 / np.sqrt(a_t), np.sqrt(1 - a_t) / np.sqrt(a_t), np.sqrt(a_p) * (1 - al) / (1 - a_t),
               np.sqrt(al) * (1 - a_p) / (1 - a_t), np.sqrt((1 - a_p) / (1 - a_t) * (1 - al))]
    return [float(np.float32(r)) for r in row]


def op_guided_step(kind, x, eps2, row, g, phi, lr=None, noise=None, clip=0.0):
    """mrisr_op_guided_step on copies: returns (new x, staging buffer [2B])."""
    import mrisr
    L = mrisr._lib
    x = x.clone()
    x2 = torch.full((2 * x.shape[0],) + tuple(x.shape[1:]), float("nan"), device=x.device)
    t = {k: L.as_tensor(v) for k, v in (("x", x), ("x2", x2), ("e", eps2), ("lr", lr), ("nz", noise)) if v is not None}
    L.check(L.lib().mrisr_op_guided_step(kind, C.byref(t["x"]), C.byref(t["x2"]), C.byref(t["e"]),
                                         C.byref(t["lr"]) if lr is not None else None, C.byref(t["nz"]) if noise is not None else None,
                                         (C.c_float * 8)(*row), clip, g, phi, L.stream_ptr()))
    return x, x2


def ref_guided_step(kind, x, eps2, row, g, phi, lr=None, noise=None, clip=0.0):
    """The formulae of include/mrisr.h in float64 on the same (f32-valued) inputs."""
    B = x.shape[0]
    x, eps2 = x.double(), eps2.double()
    e = guided_eps(eps2[:B], eps2[B:], float(np.float32(g)), float(np.float32(phi)))
    if kind == DDIM:
        return row[0] * x + row[1] * e
    if kind == RESSHIFT:
        sat, s1mat, sap, sig = row
        x0 = (x - (1 - sat) * lr.double() - s1mat * e) / sat
        v = sap * x0 + (1 - sap) * lr.double()
    else:
        ia, ie, c0, cx, sig = row
        x0 = ia * x - ie * e
        if clip > 0:
            x0 = x0.clamp(-clip, clip)
        v = c0 * x0 + cx * x
    return v + sig * noise.double() if noise is not None else v


def kernel_cases():
    for kind in (DDIM, RESSHIFT, DDPM):
        for with_noise in ((False,) if kind == DDIM else (False, True)):
            for clip in ((0.0, 1.0) if kind == DDPM else (0.0,)):
                yield kind, with_noise, clip


# (1, 4, 72): 20736 elements per sample, above the 16 Ki the registers hold - the re-reading kernel
# (2, 4, 40): 6400 elements per sample - the two-pieces-per-thread kernel (4096 < per <= 8192), 1600 pieces on 1024 threads: a masked tail
@pytest.mark.parametrize("B,Cc,h", [(1, 4, 16), (3, 4, 32), (32, 4, 32), (2, 4, 64), (8, 1, 32), (1, 4, 72), (2, 4, 40)])
def test_guided_step_kernel_matches_float64_formulae(B, Cc, h):
    gen = torch.Generator().manual_seed(7000 + B * 100 + h)
    x = torch.randn((B, Cc, h, h), generator=gen).cuda()
    eps2 = torch.randn((2 * B, Cc, h, h), generator=gen)
    eps2[B:] = 0.8 * eps2[B:] + 0.5 * eps2[:B] + 0.05  # correlated halves with a mean, as two forwards of one network give
    eps2 = eps2.cuda()
    lr = (0.3 * torch.randn((B, Cc, h, h), generator=gen)).cuda()
    nz = torch.randn((B, Cc, h, h), generator=gen).cuda()
    worst = (0.0, 0.0)
    for kind, with_noise, clip in kernel_cases():
        row = coef_row(kind)
        kw = dict(lr=lr if kind == RESSHIFT else None, noise=nz if with_noise else None, clip=clip)
        for g in (0.0, 1.0, 3.5, 7.5):
            for phi in (0.0, 0.7, 1.0):
                out, x2 = op_guided_step(kind, x, eps2, row, g, phi, **kw)
                ref = ref_guided_step(kind, x, eps2, row, g, phi, **kw)
                r, m = rel(out, ref), maxrel(out, ref)
                worst = (max(worst[0], r), max(worst[1], m))
                assert r <= 1e-5 and m <= 1e-5, (kind, with_noise, clip, g, phi, r, m)
                # the next forward's input: both halves of the staging buffer are the new state, bit for bit
                assert torch.equal(x2[:B], out) and torch.equal(x2[B:], out), (kind, g, phi)
    print(f"guided step kernel B={B} C={Cc} h={h}: worst rel {worst[0]:.3e} maxrel {worst[1]:.3e}")


@pytest.mark.parametrize("kind", [DDIM, RESSHIFT, DDPM])
def test_guided_step_kernel_constant_rows_and_sample_isolation(kind):
    gen = torch.Generator().manual_seed(7100 + kind)
    B, shape = 3, (3, 4, 32, 32)
    x = torch.randn(shape, generator=gen).cuda()
    eps2 = torch.randn((2 * B,) + shape[1:], generator=gen).cuda()
    lr = (0.3 * torch.randn(shape, generator=gen)).cuda() if kind == RESSHIFT else None
    nz = torch.randn(shape, generator=gen).cuda() if kind != DDIM else None
    row = coef_row(kind)
    base, _ = op_guided_step(kind, x, eps2, row, 3.5, 0.7, lr=lr, noise=nz)
    # statistics are per sample: replacing sample 1's eps rows (both halves) leaves samples 0 and 2 bit-identical
    other = eps2.clone()
    other[1] = 9.0 * torch.randn(shape[1:], generator=gen).cuda()
    other[B + 1] = -4.0 * torch.randn(shape[1:], generator=gen).cuda() + 2.0
    out, _ = op_guided_step(kind, x, other, row, 3.5, 0.7, lr=lr, noise=nz)
    assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2]) and not torch.equal(out[1], base[1])
    # an all-equal prediction (std 0) is left unrescaled instead of dividing by zero: finite, and the phi = 0 result
    for cu, cc in ((0.3, 0.3), (0.1, 0.7), (0.0, 0.0)):
        const = eps2.clone()
        const[0], const[B] = cu, cc
        for phi in (0.7, 1.0):
            out, x2 = op_guided_step(kind, x, const, row, 7.5, phi, lr=lr, noise=nz)
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x2).all()), (cu, cc, phi)
            plain, _ = op_guided_step(kind, x, const, row, 7.5, 0.0, lr=lr, noise=nz)
            assert maxrel(out[0], plain[0]) <= 1e-6  # the same f32 expression in another kernel: a few ulps at most
            assert maxrel(out[1:], ref_guided_step(kind, x, const, row, 7.5, phi, lr=lr, noise=nz)[1:]) <= 1e-5


# ------------------------------------------------------------------------------------------------ models
@pytest.fixture(scope="module")
def tiny():
    """TINY UNet (+ rank-4 LoRA) and ControlNet: oracle callables and one f32 device model of each."""
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=2201, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=2203))
    cp = ou.init_controlnet_params(cfg, seed=2202, perturb_norm=True)
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    unet.load_state_dict(p)
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="f32")
    cnet.load_state_dict(cp)
    return dict(cfg=cfg, p=p, cp=cp, unet=unet, cnet=cnet, o_unet=ou.OracleUNet(p, cfg), o_cnet=ou.OracleControlNet(cp, cfg))


@pytest.fixture(scope="module")
def mnist():
    import mrisr
    from oracle import unet as ou
    cfg = ou.MNIST
    p = ou.init_unet_params(cfg, seed=2211, perturb_norm=True)
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32")
    unet.load_state_dict(p)
    return dict(cfg=cfg, p=p, unet=unet, o_unet=ou.OracleUNet(p, cfg))


def contexts(cfg, B, seed):
    """A per-sample conditional context and ONE unconditional context (as the empty caption's embedding is)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, 77, cfg.cross_attention_dim), generator=g), torch.randn((B, 77, cfg.cross_attention_dim), generator=g)


def check_states(tag, make_sampler, x0, oracle_traj, n, run_kw):
    """Every state of an n-step guided run (mrisr_sampler_set_range stops the fused loop after k steps) against the oracle's."""
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
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_ddim_trajectory_with_lora(tiny, phi):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, g = tiny["cfg"], 2, 3.0
    ctx_u, ctx_c = contexts(cfg, B, 2301)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(2302))
    for n in (5, 10):
        so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
        so.set_timesteps(n)
        traj = osa.ddim_sample(GuidedUNet(tiny["o_unet"], ctx_u.expand(B, -1, -1), ctx_c, g, phi), x, None, so)
        sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
        sp.set_timesteps(n)
        kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi)
        make = lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim")  # noqa: E731
        if n == 5:
            check_states(f"ddim+lora phi={phi}", make, x.cuda(), traj, n, kw)
        else:
            check_final(f"ddim+lora n=10 phi={phi}", make, x.cuda(), traj[-1], kw)


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_res_srdiff_trajectory_with_controlnet_and_noise(tiny, phi):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, g = tiny["cfg"], 2, 3.0
    ctx_u, ctx_c = contexts(cfg, B, 2311)
    gen = torch.Generator().manual_seed(2312)
    lr_lat = 0.18215 * torch.randn((B, 4, 16, 16), generator=gen)
    cond = torch.randn((B, 3, 128, 128), generator=gen)
    init_noise = torch.randn(lr_lat.shape, generator=gen)
    for n in (5, 10):
        step_noise = torch.stack([torch.randn(lr_lat.shape, generator=gen) for _ in range(n - 1)])
        so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
        so.set_timesteps(n)
        cu = ctx_u.expand(B, -1, -1)
        traj = osa.res_srdiff_sample(GuidedUNet(tiny["o_unet"], cu, ctx_c, g, phi), GuidedControlNet(tiny["o_cnet"], cu, ctx_c), lr_lat,
                                     None, cond, so.timesteps, so.alphas_cumprod, init_noise, list(step_noise))
        sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        sp.set_timesteps(n)
        x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, init_noise.cuda())
        assert rel(x0, traj[0]) < 1e-5
        kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi,
                  lr_latents=lr_lat.cuda(), step_noise=step_noise.cuda(), controlnet_cond=cond.cuda())
        make = lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift")  # noqa: E731
        if n == 5:
            check_states(f"res-srdiff+controlnet phi={phi}", make, x0, traj, n, kw)
        else:
            check_final(f"res-srdiff+controlnet n=10 phi={phi}", make, x0, traj[-1], kw)


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_ddpm_trajectory_mnist_clip(mnist, phi):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, g, clip = mnist["cfg"], 2, 3.0, 1.0
    ctx_u, ctx_c = contexts(cfg, B, 2321)
    gen = torch.Generator().manual_seed(2322)
    x = torch.randn((B, 1, 32, 32), generator=gen)
    for n in (5, 10):
        z = torch.randn((n, B, 1, 32, 32), generator=gen)
        so = osch.OracleScheduler(beta_start=1e-4, beta_end=0.02, beta_schedule="linear")
        so.set_timesteps(n)
        traj = osa.ddpm_sample(GuidedUNet(mnist["o_unet"], ctx_u.expand(B, -1, -1), ctx_c, g, phi), x, None, so, z, clip)
        sp = mrisr.DDPMScheduler(beta_start=1e-4, beta_end=0.02, beta_schedule="linear")
        sp.set_timesteps(n)
        kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi,
                  step_noise=z.cuda())
        make = lambda: mrisr.Sampler(mnist["unet"], sp, kind="ddpm", clip_sample_range=clip)  # noqa: E731
        if n == 5:
            check_states(f"ddpm mnist clip phi={phi}", make, x.cuda(), traj, n, kw)
        else:
            check_final(f"ddpm mnist clip n=10 phi={phi}", make, x.cuda(), traj[-1], kw)


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_ddim_trajectory_with_adapter_features(tiny, golden_dir, phi):
    import mrisr
    from oracle import adapter as oad
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, g = tiny["cfg"], 2, 3.0
    gold = np.load(os.path.join(golden_dir, "adapter_xl.npz"))
    feats = oad.adapter_forward(oad.init_adapter_params(oad.ADAPTER_TINY, seed=401), oad.ADAPTER_TINY, torch.from_numpy(gold["x"]))
    assert feats[0].shape[0] == B
    ctx_u, ctx_c = contexts(cfg, B, 2331)
    x = torch.randn((B, 4, 8, 8), generator=torch.Generator().manual_seed(2332))
    for n in (5, 10):
        so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
        so.set_timesteps(n)
        traj = osa.ddim_sample(GuidedUNet(tiny["o_unet"], ctx_u.expand(B, -1, -1), ctx_c, g, phi), x, None, so,
                               intrablock=[f.clone() for f in feats])
        sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
        sp.set_timesteps(n)
        kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi,
                  adapter_features=[f.cuda() for f in feats])
        make = lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim")  # noqa: E731
        if n == 5:
            check_states(f"ddim+adapter phi={phi}", make, x.cuda(), traj, n, kw)
        else:
            check_final(f"ddim+adapter n=10 phi={phi}", make, x.cuda(), traj[-1], kw)


# ------------------------------------------------------------------------------------------------ 3.-6. the sampler's state
def resshift_setup(tiny, B=2, n=5, seed=2341):
    import mrisr
    gen = torch.Generator().manual_seed(seed)
    lr_lat = (0.18215 * torch.randn((B, 4, 16, 16), generator=gen)).cuda()
    sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    x0 = mrisr.get_res_shifting_latents(lr_lat, lr_lat, sp.timesteps[0], sp, torch.randn(lr_lat.shape, generator=gen).cuda())
    ctx_u, ctx_c = contexts(tiny["cfg"], B, seed + 1)
    kw = dict(encoder_hidden_states=ctx_c.cuda(), lr_latents=lr_lat,
              step_noise=torch.stack([torch.randn(lr_lat.shape, generator=gen) for _ in range(n - 1)]).cuda(),
              controlnet_cond=torch.randn((B, 3, 128, 128), generator=gen).cuda())
    return sp, x0, ctx_u.cuda(), kw


def test_guided_graph_replay_equals_eager_launches(tiny):
    import mrisr
    sp, x0, ctx_u, kw = resshift_setup(tiny)
    finals = {}
    for use_graph in (True, False):
        lat = x0.clone().contiguous()
        mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift").run(lat, uncond_hidden_states=ctx_u, guidance_scale=3.0,
                                                                           guidance_rescale=0.7, use_graph=use_graph, **kw)
        torch.cuda.synchronize()
        finals[use_graph] = lat.cpu()
    assert torch.equal(finals[True], finals[False])
    assert not torch.equal(finals[True], x0.cpu())


@pytest.mark.parametrize("kind", ["ddim", "resshift", "ddpm"])
def test_guidance_scale_one_is_the_unguided_call(tiny, kind):
    """Off means off: g = 1 with an unconditional context takes the unguided path (no 2B forward), bit for bit."""
    import mrisr
    B, n = 2, 4
    gen = torch.Generator().manual_seed(2351)
    ctx_u, ctx_c = contexts(tiny["cfg"], B, 2352)
    x = torch.randn((B, 4, 16, 16), generator=gen).cuda()
    sp = (mrisr.DDIMScheduler if kind == "ddim" else mrisr.DDPMScheduler)(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    kw = {}
    if kind == "resshift":
        kw["lr_latents"] = (0.2 * torch.randn((B, 4, 16, 16), generator=gen)).cuda()
    if kind != "ddim":
        kw["step_noise"] = torch.randn((n, B, 4, 16, 16), generator=gen).cuda()
    a, b = x.clone(), x.clone()
    mrisr.Sampler(tiny["unet"], sp, kind=kind).run(a, ctx_c.cuda(), **kw)
    smp = mrisr.Sampler(tiny["unet"], sp, kind=kind)
    smp.run(b, ctx_c.cuda(), guidance_scale=1.0, guidance_rescale=0.0, uncond_hidden_states=ctx_u.cuda(), **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, x)
    assert smp._keep[0].shape[0] == B  # the context it handed to the library has B rows: no 2B forward


def test_guidance_state_does_not_go_stale_on_one_sampler(tiny):
    import mrisr
    B, n = 2, 3
    gen = torch.Generator().manual_seed(2361)
    ctx_u, ctx_c = contexts(tiny["cfg"], B, 2362)
    x = torch.randn((B, 4, 16, 16), generator=gen).cuda()
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)

    def run(smp, g):
        lat = x.clone()
        if g is None:
            smp.run(lat, ctx_c.cuda())
        else:
            smp.run(lat, ctx_c.cuda(), guidance_scale=g, guidance_rescale=0.7, uncond_hidden_states=ctx_u.cuda())
        torch.cuda.synchronize()
        return lat.cpu()

    one = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    seq = (3.0, 5.0, None, 3.0)
    got = [run(one, g) for g in seq]
    for g, have in zip(seq, got):
        assert torch.equal(have, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), g)), g
    assert torch.equal(got[0], got[3])
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2]) and not torch.equal(got[1], got[2])


def test_degenerate_guidance_is_the_unguided_run(tiny):
    """uncond == cond: e = eps_c in exact arithmetic for every g; the 2B forward may pick other tiles than the B forward, so
    close (1e-4), not bitwise."""
    import mrisr
    B, n = 2, 5
    _, ctx_c = contexts(tiny["cfg"], B, 2372)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(2371)).cuda()
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    a, b = x.clone(), x.clone()
    mrisr.Sampler(tiny["unet"], sp, kind="ddim").run(a, ctx_c.cuda())
    mrisr.Sampler(tiny["unet"], sp, kind="ddim").run(b, ctx_c.cuda(), guidance_scale=7.5, uncond_hidden_states=ctx_c.cuda())
    torch.cuda.synchronize()
    r = rel(b, a)
    print(f"degenerate guidance (uncond == cond, g = 7.5) vs the unguided run: rel {r:.3e}")
    assert r < 1e-4, r


# ------------------------------------------------------------------------------------------------ 7. bf16
def test_guided_ddim_step_bf16(tiny):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, g = tiny["cfg"], 2, 2.0
    ctx_u, ctx_c = contexts(cfg, B, 2381)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(2382))
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(5)
    wrapped = GuidedUNet(tiny["o_unet"], ctx_u.expand(B, -1, -1), ctx_c, g, 0.0)
    t0 = int(so.timesteps[0])
    e_ref = wrapped(x, torch.tensor(t0)).sample
    x1_ref = so.ddim_step(e_ref, t0, x)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(5)
    smp = mrisr.Sampler(net, sp, kind="ddim")
    smp.set_range(0, 1)
    lat = x.cuda().clone()
    smp.run(lat, ctx_c.cuda(), guidance_scale=g, uncond_hidden_states=ctx_u.cuda())
    torch.cuda.synchronize()
    cx, ce = so.ddim_coeffs(t0)
    e_dev = (lat.double().cpu() - cx * x.double()) / ce  # the guided prediction the step consumed
    r_x, r_e = rel(lat, x1_ref), rel(e_dev, e_ref)
    print(f"bf16 guided DDIM step, g = 2: state rel {r_x:.3e}, guided eps rel {r_e:.3e} (bound {3 * 5e-2})")
    assert r_x < 3 * 5e-2 and r_e < 3 * 5e-2, (r_x, r_e)


# ------------------------------------------------------------------------------------------------ 9. log_validation / fit
class _StubVAE:
    class config:
        scaling_factor = 0.18215

    def encode(self, x):
        z = torch.nn.functional.avg_pool2d(x[:, :1], 8).repeat(1, 4, 1, 1)
        return type("E", (), {"latent_dist": type("D", (), {"sample": staticmethod(lambda: z)})})

    def decode(self, z):
        return type("O", (), {"sample": torch.nn.functional.interpolate(z.mean(1, keepdim=True), scale_factor=8.0, mode="nearest")})


def test_log_validation_with_guidance_equals_the_pipeline_by_hand(tiny):
    import mrisr
    cfg, n, g, phi = tiny["cfg"], 3, 3.0, 0.7
    gen = torch.Generator().manual_seed(2391)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(256, 256), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    ctx_u, ctx_c = contexts(cfg, 1, 2392)
    vae, acc = _StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(2393)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(tiny["unet"], None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx_c.cuda(),
                                               num_inference_steps=n, **kw))

    got = panel(guidance_scale=g, guidance_rescale=phi, uncond_embeds=ctx_u.cuda())
    # by hand: the same draws from the same global stream, in the same order
    torch.manual_seed(2393)
    sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    lr_d = lr.cuda()
    anchor = (vae.encode(lr_d.expand(-1, 3, -1, -1)).latent_dist.sample() * vae.config.scaling_factor).float()
    sched.set_timesteps(n, device="cuda")
    lat = mrisr.get_res_shifting_latents(anchor, anchor, sched.timesteps[0], sched).contiguous()
    noise = torch.stack([torch.randn_like(lat) for _ in range(n - 1)])
    mrisr.Sampler(tiny["unet"], sched, None, kind="resshift").run(lat, ctx_c.cuda(), lr_latents=anchor, step_noise=noise, guidance_scale=g,
                                                                  guidance_rescale=phi, uncond_hidden_states=ctx_u.cuda())
    W = got.shape[1] // 3
    assert np.array_equal(got[:, W:2 * W], mrisr.decode_to_vis(lat, vae))
    assert np.array_equal(got[:, :W], mrisr.decode_to_vis(lr_d, vae, is_latent=False))
    # the arguments do something, and their defaults nothing
    plain = panel()
    assert not np.array_equal(plain[:, W:2 * W], got[:, W:2 * W])
    assert np.array_equal(plain, panel(guidance_scale=1.0, guidance_rescale=0.0, uncond_embeds=None))


def test_fit_validates_with_guidance(tmp_path):
    """fit(validation_guidance_scale=...) samples its validation panel against caption_embeds[""]: the panel of a guided run is
    the one log_validation gives with the same arguments after the same training, and not the unguided one."""
    import mrisr
    from oracle import unet as ou
    from oracle import vae as ov
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=301, perturb_norm=True)
    up.update(ou.init_lora_params(up, rank=4, seed=302))
    vp = ov.init_vae_params(ov.TINY_VAE, seed=303)
    g = torch.Generator().manual_seed(304)
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(64.0), indexing="ij")
    items = []
    for i in range(8):
        hr = (torch.sin(xx / (3 + i % 7)) * torch.cos(yy / (4 + i % 5)) + 0.1 * torch.randn((64, 64), generator=g)).clamp(-1, 1)
        lr = torch.nn.functional.avg_pool2d(hr[None, None], 4).repeat_interleave(4, 2).repeat_interleave(4, 3)[0]
        items.append({"hr": hr[None], "lr": lr, "txt": "an axial T2 slice"})
    embeds = {p: torch.randn((16, cfg.cross_attention_dim), generator=g) for p in ("", "an axial T2 slice")}
    panels = {}
    for tag, kw in (("plain", {}), ("guided", dict(validation_guidance_scale=3.0, validation_guidance_rescale=0.7))):
        unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4, lora_fused=True)
        unet.load_state_dict(up)
        vae = mrisr.AutoencoderKL(ov.TINY_VAE, compute_dtype="f32")
        vae.load_state_dict(vp)
        conf = mrisr.TrainConfig(output_dir=str(tmp_path / tag), resolution=64, train_batch_size=2, gradient_accumulation_steps=1,
                                 max_train_steps=2, learning_rate=1e-3, lr_warmup_steps=1, logging_steps=1, validation_steps=2,
                                 checkpointing_steps=1000, mixed_precision="no", proportion_empty_prompts=0.1, seed=1234)
        torch.manual_seed(77)
        res = mrisr.fit(conf, unet, vae, items, embeds, val_dataset=items[:1], **kw)
        assert len(res.validation_paths) == 1
        from PIL import Image
        panels[tag] = np.asarray(Image.open(res.validation_paths[0]))
    W = panels["plain"].shape[1] // 3
    assert np.array_equal(panels["plain"][:, :W], panels["guided"][:, :W])            # same LR / HR columns
    assert not np.array_equal(panels["plain"][:, W:2 * W], panels["guided"][:, W:2 * W])  # another sample in the middle


# ------------------------------------------------------------------------------------------------ 10. errors
def test_guidance_errors_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    B, n = 2, 3
    gen = torch.Generator().manual_seed(2401)
    ctx_u, ctx_c = contexts(tiny["cfg"], B, 2402)
    x = torch.randn((B, 4, 16, 16), generator=gen).cuda()
    sp = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="resshift")
    lr = torch.zeros_like(x)
    lat = x.clone()
    bad = [dict(guidance_scale=3.0),                                                                   # no unconditional context
           dict(guidance_scale=3.0, guidance_rescale=1.5, uncond_hidden_states=ctx_u.cuda()),         # rescale outside [0, 1]
           dict(guidance_scale=3.0, guidance_rescale=-0.5, uncond_hidden_states=ctx_u.cuda()),
           dict(guidance_rescale=0.7),                                                                 # rescale without guidance
           dict(guidance_scale=1.0, guidance_rescale=0.7, uncond_hidden_states=ctx_u.cuda()),
           dict(guidance_scale=3.0, uncond_hidden_states=ctx_u[:, :76].cuda()),                        # L mismatch
           dict(guidance_scale=3.0, uncond_hidden_states=ctx_u[:, :, :32].cuda()),                     # D mismatch
           dict(guidance_scale=3.0, uncond_hidden_states=torch.cat([ctx_u] * 3).cuda()),               # rows
           dict(guidance_scale=3.0, uncond_hidden_states=ctx_u.cuda(), adapter_features=[torch.zeros((1, 64, 16, 16)).cuda()])]
    for kw in bad:
        with pytest.raises(ValueError):
            smp.run(lat, ctx_c.cuda(), lr_latents=lr, **kw)
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran

    # the C ABI validates every operand against B / 2B itself (its kernels index without bounds)
    ehs2 = torch.cat([ctx_u.expand(B, -1, -1), ctx_c]).cuda().contiguous()
    noise = torch.randn((n - 1, B, 4, 16, 16), generator=gen).cuda()

    def run_guided(ehs, feats=(), nz=noise):
        t_lat, t_lr, t_e = L.as_tensor(lat), L.as_tensor(lr), L.as_tensor(ehs)
        t_nz = L.as_tensor(nz, shape=(nz.shape[0] * nz.shape[1],) + tuple(nz.shape[2:]))
        f_arr = L.tensor_array([L.as_tensor(f) for f in feats])
        L.check(L.lib().mrisr_sampler_set_guidance(smp._h, 3.0, 0.0))
        L.check(L.lib().mrisr_sampler_run_guided(smp._h, C.byref(t_lat), C.byref(t_lr), C.byref(t_nz), C.byref(t_e), None,
                                                 f_arr if feats else None, len(feats), 1, L.stream_ptr()))

    with pytest.raises(RuntimeError, match="encoder_hidden_states"):
        run_guided(ctx_c.cuda().contiguous())                                    # [B] rows where 2B are needed
    with pytest.raises(RuntimeError, match="adapter features"):
        run_guided(ehs2, feats=[torch.zeros((B, 64, 16, 16)).cuda()])            # a [B] feature in a guided run
    with pytest.raises(RuntimeError, match="step_noise"):
        run_guided(ehs2, nz=noise[:1].contiguous())                              # a short noise stack
    with pytest.raises(RuntimeError, match="guidance_rescale"):
        L.check(L.lib().mrisr_sampler_set_guidance(smp._h, 3.0, 1.5))
    torch.cuda.synchronize()
    assert torch.equal(lat, x)
    run_guided(ehs2)  # and the well-formed call runs
    torch.cuda.synchronize()
    assert not torch.equal(lat, x) and bool(torch.isfinite(lat).all())


# ------------------------------------------------------------------------------------------------ 8. SD-1.5 width (last: the expensive one)
def test_zz_guided_ddim_sd15_width():
    """Full SD-1.5 width, f32, B = 1, two guided DDIM steps with rescale against the wrapped full-width oracle (4 oracle
    forwards).  Builds its own f32 engine (the full-width fixtures of test_gpu_fullwidth.py are module-scoped there) and frees it."""
    import gc

    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    from oracle import unet as ou
    cfg = ou.SD15
    p = ou.init_unet_params(cfg, seed=1101, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=1103))
    B, g, phi = 1, 3.0, 0.7
    ctx_u, ctx_c = contexts(cfg, B, 2411)
    x = torch.randn((B, 4, 32, 32), generator=torch.Generator().manual_seed(2412))
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(2)
    traj = osa.ddim_sample(GuidedUNet(ou.OracleUNet(p, cfg), ctx_u, ctx_c, g, phi), x, None, so)
    net = mrisr.UNet2DConditionModel(mrisr.UNetConfig(), compute_dtype="f32", lora_rank=4, lora_alpha=4, lora_fused=True,
                                     flash_attention=True)
    net.load_state_dict(p)
    sp = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(2)
    lat = x.cuda().clone()
    smp = mrisr.Sampler(net, sp, kind="ddim")
    smp.run(lat, ctx_c.cuda(), guidance_scale=g, guidance_rescale=phi, uncond_hidden_states=ctx_u.cuda())
    torch.cuda.synchronize()
    r, m = rel(lat, traj[-1]), maxrel(lat, traj[-1])
    del smp, net, p
    gc.collect()
    torch.cuda.empty_cache()
    print(f"SD-1.5 width guided DDIM x2 (g = 3, phi = 0.7) vs the wrapped oracle: rel {r:.3e} maxrel {m:.3e}")
    assert r < 1e-3, (r, m)
