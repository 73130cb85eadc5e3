"""GPU: perturbed-attention guidance (PAG) in the graph sampler against the patched CPU oracle (tests/pag_ref.py, itself checked by
test_pag_cpu.py): the perturbed prediction of a single forward, trajectories of all five step kinds, PAG with classifier-free
guidance, ControlNet, adapter features, tiles, graph == eager, "off means off", no stale model state, bf16, SD-1.5 width,
``log_validation`` plumbing and the refusals.  TINY UNet (+ rank-4 LoRA), f32 engine, B = 2, 16 x 16 latents unless stated.

Tolerances: f32 1e-3 relative L2 and max-relative (the f32 tolerance of every sampler test here).  bf16: the single-forward bound
5e-2 amplified as test_gpu_guidance.py derives it - the combined prediction (1 + s) eps_c - s eps_p carries 1 + 2 s times the
single-forward error, and g eps_c - (g - 1) eps_u adds 2 (g - 1): 5e-2 (1 + 2 s) for PAG alone, 5e-2 (1 + 2 (g - 1) + 2 s) with CFG.
``mid`` alone moves the prediction by 1e-2 only (test_pag_cpu.py), below bf16's bound: every bf16 test and every "the perturbation
is real" assertion uses ``down_blocks.0`` / ``up_blocks.3`` or all layers."""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

from guidance_ref import GuidedControlNet
from pag_ref import CtxControlNet, PagUNet, block_names, mask_of, perturbed_attention
from pag_testlib import StubVAE, maxrel, rel
from tiles_ref import TiledUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ALL = ("down_blocks", "mid", "up_blocks")
OUTER = ("down_blocks.0", "up_blocks.3")


@pytest.fixture(scope="module")
def tiny():
    """TINY UNet (+ rank-4 LoRA) and ControlNet as test_gpu_guidance.py builds them."""
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


def contexts(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, 77, cfg.cross_attention_dim), generator=g), torch.randn((B, 77, cfg.cross_attention_dim), generator=g)


def host_scheduler(kind, n):
    import mrisr
    cls = {"ddim": mrisr.DDIMScheduler, "resshift": mrisr.DDPMScheduler, "ddpm": mrisr.DDPMScheduler,
           "unipc": mrisr.UniPCMultistepScheduler, "dpmsolver++": mrisr.DPMSolverMultistepScheduler}[kind]
    sp = cls(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    return sp


def check_states(tag, make_sampler, x0, traj, n, run_kw, tol=1e-3):
    """Every state of an n-step run (set_range stops the fused loop after k steps) against the oracle's."""
    smp = make_sampler()
    for k in range(1, n + 1):
        lat = x0.clone().contiguous()
        smp.set_range(0, k)
        smp.run(lat, **run_kw)
        torch.cuda.synchronize()
        r, m = rel(lat, traj[k]), maxrel(lat, traj[k])
        print(f"{tag}: state {k}/{n} rel {r:.3e} maxrel {m:.3e}")
        assert r < tol and m < tol, (tag, k, r, m)


# ------------------------------------------------------------------------------------------------ 1. one forward
def single_forward(unet, o_unet, cfg, layers, seed, hw=16):
    """Rows 0 and 1 carry identical inputs; the model's PAG state perturbs row 0 only.  Returns (device out [2], oracle perturbed
    [1], oracle plain [1])."""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn((1, 4, hw, hw), generator=g)
    ctx1 = torch.randn((1, 77, cfg.cross_attention_dim), generator=g)
    t = torch.tensor(500)
    names = unet.transformer_block_names()
    assert names == block_names(cfg)
    unet.set_pag(mask_of(layers, names), 0, 1)
    try:
        out = unet(x1.repeat(2, 1, 1, 1).cuda(), t, encoder_hidden_states=ctx1.repeat(2, 1, 1).cuda()).sample
        torch.cuda.synchronize()
    finally:
        unet.set_pag()
    plain = o_unet(x1, t, encoder_hidden_states=ctx1).sample
    with perturbed_attention(layers):
        pert = o_unet(x1, t, encoder_hidden_states=ctx1).sample
    return out.cpu(), pert, plain


@pytest.mark.parametrize("layers", [("mid",), OUTER, ALL], ids=["mid", "outer", "all"])
def test_single_forward_perturbs_exactly_the_selected_rows(tiny, layers):
    out, pert, plain = single_forward(tiny["unet"], tiny["o_unet"], tiny["cfg"], layers, 2801)
    r0, m0, r1, m1 = rel(out[:1], pert), maxrel(out[:1], pert), rel(out[1:], plain), maxrel(out[1:], plain)
    moved, want = rel(out[:1], out[1:]), rel(pert, plain)
    print(f"PAG forward {layers}: perturbed row rel {r0:.3e} maxrel {m0:.3e}; plain row rel {r1:.3e} maxrel {m1:.3e}; rows differ by "
          f"{moved:.3e} (oracle {want:.3e})")
    assert r0 <= 1e-3 and m0 <= 1e-3 and r1 <= 1e-3 and m1 <= 1e-3
    assert 0.9 * want <= moved <= 1.1 * want
    # the state is gone: the same call is the plain forward on both rows again
    g = torch.Generator().manual_seed(2801)
    x1 = torch.randn((1, 4, 16, 16), generator=g)
    ctx1 = torch.randn((1, 77, tiny["cfg"].cross_attention_dim), generator=g)
    both = tiny["unet"](x1.repeat(2, 1, 1, 1).cuda(), torch.tensor(500), encoder_hidden_states=ctx1.repeat(2, 1, 1).cuda()).sample.cpu()
    assert rel(both[:1], plain) <= 1e-3 and rel(both[1:], plain) <= 1e-3


def test_single_forward_sd15_width():
    """Full SD-1.5 width, f32, B = 2 on ("mid",): head dim 160 runs inside the model.  Builds its own engine and frees it before it
    returns, so it does not matter where in the file's order it runs."""
    import mrisr
    from oracle import unet as ou
    cfg = ou.SD15
    p = ou.init_unet_params(cfg, seed=1101, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=1103))
    net = mrisr.UNet2DConditionModel(mrisr.UNetConfig(), compute_dtype="f32", lora_rank=4, lora_alpha=4, lora_fused=True, flash_attention=True)
    net.load_state_dict(p)
    out, pert, plain = single_forward(net, ou.OracleUNet(p, cfg), cfg, ("mid",), 2811)
    del net, p
    gc.collect()
    torch.cuda.empty_cache()
    r0, r1, moved, want = rel(out[:1], pert), rel(out[1:], plain), rel(out[:1], out[1:]), rel(pert, plain)
    print(f"SD-1.5 width PAG forward (mid): perturbed row rel {r0:.3e}, plain row rel {r1:.3e}; rows differ by {moved:.3e} (oracle {want:.3e})")
    assert r0 <= 1e-3 and r1 <= 1e-3
    assert 0.9 * want <= moved <= 1.1 * want


# ------------------------------------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("kind", ["ddim", "resshift", "ddpm", "unipc", "dpmsolver++"])
def test_pag_alone_trajectory(tiny, kind):
    import mrisr
    import multistep_ref as mref
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n, s = tiny["cfg"], 2, 5, 2.0
    _, ctx = contexts(cfg, B, 2821)
    gen = torch.Generator().manual_seed(2822)
    x = torch.randn((B, 4, 16, 16), generator=gen)
    lr_lat = 0.18215 * torch.randn((B, 4, 16, 16), generator=gen)
    init_noise = torch.randn(x.shape, generator=gen)
    z = torch.randn((n, B, 4, 16, 16), generator=gen)
    wrapped = PagUNet(tiny["o_unet"], ctx, s, OUTER)
    sp = host_scheduler(kind, n)
    kw = dict(encoder_hidden_states=ctx.cuda(), pag_scale=s, pag_applied_layers=OUTER)
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    x0 = x.cuda()
    if kind == "ddim":
        traj = osa.ddim_sample(wrapped, x, None, so)
    elif kind == "ddpm":
        traj = osa.ddpm_sample(wrapped, x, None, so, z, 0.0)
        kw["step_noise"] = z.cuda()
    elif kind == "resshift":
        traj = osa.res_srdiff_sample(wrapped, None, lr_lat, None, None, so.timesteps, so.alphas_cumprod, init_noise, list(z[:n - 1]))
        x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, init_noise.cuda())
        kw.update(lr_latents=lr_lat.cuda(), step_noise=z[:n - 1].cuda())
    else:
        traj = mref.multistep_sample(kind, wrapped, x, None, sp.timesteps, sp.alphas_cumprod, lr_latents=lr_lat, last=n)
        kw["lr_latents"] = lr_lat.cuda()
    check_states(f"pag alone {kind}", lambda: mrisr.Sampler(tiny["unet"], sp, kind=kind), x0, traj, n, kw)


@pytest.mark.parametrize("kind", ["ddim", "resshift", "unipc", "dpmsolver++"])
def test_pag_with_cfg_and_rescale_trajectory(tiny, kind):
    import mrisr
    import multistep_ref as mref
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n, g, s, phi = tiny["cfg"], 2, 5, 3.0, 1.5, 0.7
    ctx_u, ctx_c = contexts(cfg, B, 2831)
    gen = torch.Generator().manual_seed(2832)
    x = torch.randn((B, 4, 16, 16), generator=gen)
    lr_lat = 0.18215 * torch.randn((B, 4, 16, 16), generator=gen)
    init_noise = torch.randn(x.shape, generator=gen)
    z = torch.randn((n - 1, B, 4, 16, 16), generator=gen)
    wrapped = PagUNet(tiny["o_unet"], ctx_c, s, ALL, ctx_u=ctx_u.expand(B, -1, -1), guidance_scale=g, guidance_rescale=phi)
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    sp = host_scheduler(kind, n)
    kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi, pag_scale=s,
              pag_applied_layers=ALL)
    if kind == "ddim":
        traj, x0 = osa.ddim_sample(wrapped, x, None, so), x.cuda()
    elif kind in ("unipc", "dpmsolver++"):  # the three-way step with the history ring (and UniPC's corrected state), LR-anchored
        traj, x0 = mref.multistep_sample(kind, wrapped, x, None, sp.timesteps, sp.alphas_cumprod, lr_latents=lr_lat, last=n), x.cuda()
        kw["lr_latents"] = lr_lat.cuda()
    else:
        traj = osa.res_srdiff_sample(wrapped, None, lr_lat, None, None, so.timesteps, so.alphas_cumprod, init_noise, list(z))
        x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, init_noise.cuda())
        kw.update(lr_latents=lr_lat.cuda(), step_noise=z.cuda())
    check_states(f"pag + cfg + rescale {kind}", lambda: mrisr.Sampler(tiny["unet"], sp, kind=kind), x0, traj, n, kw)


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_pag_with_cfg_multistep_trajectory_without_rescale(tiny, kind):
    """phi = 0: the grid-stride form of the three-way step with the ring; UniPC at order 3."""
    import mrisr
    import multistep_ref as mref
    cfg, B, n, g, s = tiny["cfg"], 2, 5, 3.0, 1.5
    order = 3 if kind == "unipc" else 2
    ctx_u, ctx_c = contexts(cfg, B, 2835)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(2836))
    wrapped = PagUNet(tiny["o_unet"], ctx_c, s, OUTER, ctx_u=ctx_u.expand(B, -1, -1), guidance_scale=g)
    sp = host_scheduler(kind, n)
    traj = mref.multistep_sample(kind, wrapped, x, None, sp.timesteps, sp.alphas_cumprod, solver_order=order, last=n)

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind=kind)
        smp.set_solver(order)
        return smp

    kw = dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, pag_scale=s, pag_applied_layers=OUTER)
    check_states(f"pag + cfg {kind} order {order}", make, x.cuda(), traj, n, kw)


@pytest.mark.parametrize("with_cfg", [False, True], ids=["pag", "pag+cfg"])
def test_pag_trajectory_with_controlnet(tiny, with_cfg):
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n, g, s = tiny["cfg"], 2, 5, 3.0, 2.0
    ctx_u, ctx_c = contexts(cfg, B, 2841)
    cu = ctx_u.expand(B, -1, -1)
    gen = torch.Generator().manual_seed(2842)
    lr_lat = 0.18215 * torch.randn((B, 4, 16, 16), generator=gen)
    cond = torch.randn((B, 3, 128, 128), generator=gen)
    init_noise = torch.randn(lr_lat.shape, generator=gen)
    z = torch.randn((n - 1, B, 4, 16, 16), generator=gen)
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    if with_cfg:
        wrapped, o_cnet = PagUNet(tiny["o_unet"], ctx_c, s, OUTER, ctx_u=cu, guidance_scale=g), GuidedControlNet(tiny["o_cnet"], cu, ctx_c)
    else:
        wrapped, o_cnet = PagUNet(tiny["o_unet"], ctx_c, s, OUTER), CtxControlNet(tiny["o_cnet"], ctx_c)
    traj = osa.res_srdiff_sample(wrapped, o_cnet, lr_lat, None, cond, so.timesteps, so.alphas_cumprod, init_noise, list(z))
    sp = host_scheduler("resshift", n)
    x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, init_noise.cuda())
    kw = dict(encoder_hidden_states=ctx_c.cuda(), lr_latents=lr_lat.cuda(), step_noise=z.cuda(), controlnet_cond=cond.cuda(), pag_scale=s,
              pag_applied_layers=OUTER)
    if with_cfg:
        kw.update(uncond_hidden_states=ctx_u.cuda(), guidance_scale=g)
    check_states(f"pag + controlnet cfg={with_cfg}", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift"), x0, traj, n, kw)


def test_pag_trajectory_with_adapter_features(tiny, golden_dir):
    import mrisr
    from oracle import adapter as oad
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n, s = tiny["cfg"], 2, 5, 2.0
    gold = np.load(os.path.join(golden_dir, "adapter_xl.npz"))
    feats = oad.adapter_forward(oad.init_adapter_params(oad.ADAPTER_TINY, seed=401), oad.ADAPTER_TINY, torch.from_numpy(gold["x"]))
    assert feats[0].shape[0] == B
    _, ctx = contexts(cfg, B, 2851)
    x = torch.randn((B, 4, 8, 8), generator=torch.Generator().manual_seed(2852))
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    traj = osa.ddim_sample(PagUNet(tiny["o_unet"], ctx, s, OUTER), x, None, so, intrablock=[f.clone() for f in feats])
    sp = host_scheduler("ddim", n)
    kw = dict(encoder_hidden_states=ctx.cuda(), adapter_features=[f.cuda() for f in feats], pag_scale=s, pag_applied_layers=OUTER)
    check_states("pag + adapter", lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), traj, n, kw)


@pytest.mark.parametrize("with_cfg", [False, True], ids=["pag", "pag+cfg"])
def test_pag_with_tiles(tiny, with_cfg):
    """B = 2 on a 32 x 32 canvas, tile 16, overlap 8 (T = 9): sample b owns tile rows b T .. b T + T - 1 and the perturbed range is
    [0, B T), with CFG the first third of 3 B T rows.  The reference composes tests/tiles_ref.py (the wrapped network runs on the tile
    batch and blends) with PagUNet (which combines the blended canvas predictions).  Two distinct per-sample contexts and 3 steps:
    a row given to the wrong sample, or a perturbed range one sample short, misses 1e-3 by orders of magnitude."""
    import mrisr
    from oracle import sampler as osa
    from oracle import schedulers as osch
    cfg, B, n, s, g = tiny["cfg"], 2, 3, 2.0, 3.0
    ctx_u, ctx = contexts(cfg, B, 2861)
    x = torch.randn((B, 4, 32, 32), generator=torch.Generator().manual_seed(2862))
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    extra = dict(ctx_u=ctx_u.expand(B, -1, -1), guidance_scale=g, guidance_rescale=0.7) if with_cfg else {}
    traj = osa.ddim_sample(PagUNet(TiledUNet(tiny["o_unet"], 32, 32, 16, 8), ctx, s, OUTER, **extra), x, None, so)
    sp = host_scheduler("ddim", n)

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_tiles(16, 8)
        return smp

    kw = dict(encoder_hidden_states=ctx.cuda(), pag_scale=s, pag_applied_layers=OUTER)
    if with_cfg:
        kw.update(uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=0.7)
    check_states(f"pag + tiles cfg={with_cfg}", make, x.cuda(), traj, n, kw)


# ------------------------------------------------------------------------------------------------ 3. the sampler's state
def ddim_setup(tiny, B=2, n=4, seed=2871):
    _, ctx = contexts(tiny["cfg"], B, seed)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(seed + 1)).cuda()
    return host_scheduler("ddim", n), x, ctx.cuda()


def captures(smp):
    import mrisr
    return int(mrisr._lib.lib().mrisr_sampler_num_captures(smp._h))


def test_pag_graph_replay_equals_eager_launches(tiny):
    import mrisr
    sp, x, ctx = ddim_setup(tiny)
    ctx_u = contexts(tiny["cfg"], 2, 2873)[0].cuda()
    for kw in (dict(pag_scale=2.0, pag_applied_layers=ALL),
               dict(pag_scale=2.0, pag_applied_layers=ALL, uncond_hidden_states=ctx_u, guidance_scale=3.0, guidance_rescale=0.7)):
        finals = {}
        for use_graph in (True, False):
            lat = x.clone()
            smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
            smp.run(lat, ctx, use_graph=use_graph, **kw)
            torch.cuda.synchronize()
            finals[use_graph] = lat.cpu()
            assert captures(smp) == (1 if use_graph else 0)
        assert torch.equal(finals[True], finals[False]) and not torch.equal(finals[True], x.cpu())


def test_pag_scale_zero_is_the_call_without_it(tiny):
    """Off means off: the same bits and the same number of graph captures, also for a guided run."""
    import mrisr
    sp, x, ctx = ddim_setup(tiny)
    ctx_u = contexts(tiny["cfg"], 2, 2875)[0].cuda()
    for extra in ({}, dict(uncond_hidden_states=ctx_u, guidance_scale=3.0, guidance_rescale=0.7)):
        a, b = x.clone(), x.clone()
        sa, sb = mrisr.Sampler(tiny["unet"], sp, kind="ddim"), mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        for _ in range(2):  # the second run replays the first one's graph in both samplers
            a.copy_(x), b.copy_(x)
            sa.run(a, ctx, **extra)
            sb.run(b, ctx, pag_scale=0.0, pag_applied_layers=ALL, **extra)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and not torch.equal(a, x)
        assert captures(sa) == captures(sb) == 1
        assert sb._keep[0].shape[0] == (2 if not extra else 4)  # no extra rows went to the library


def test_pag_leaves_no_state_behind_and_recaptures_on_change(tiny):
    import mrisr
    sp, x, ctx = ddim_setup(tiny)

    def run(smp, **kw):
        lat = x.clone()
        smp.run(lat, ctx, **kw)
        torch.cuda.synchronize()
        return lat.cpu()

    fresh = lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim")  # noqa: E731
    one = fresh()
    seq = (dict(pag_scale=2.0, pag_applied_layers=OUTER), dict(pag_scale=3.0, pag_applied_layers=OUTER),
           dict(pag_scale=3.0, pag_applied_layers=ALL), {}, dict(pag_scale=2.0, pag_applied_layers=OUTER))
    got = [run(one, **kw) for kw in seq]
    assert captures(one) == 5  # every change of the PAG configuration captured again
    again = run(one, **seq[4])  # the same configuration twice in a row: the graph is replayed
    assert torch.equal(again, got[4]) and captures(one) == 5
    for kw, have in zip(seq, got):
        assert torch.equal(have, run(fresh(), **kw)), kw  # a PAG run followed by a plain run equals a fresh plain run, and so on
    assert torch.equal(got[0], got[4])
    assert len({tuple(g.flatten()[:64].tolist()) for g in got[:4]}) == 4  # scale, layers and "off" all change the result
    # an error inside a PAG run (a feature of the wrong size meets the encoder, after the model's state was set) clears the state too
    L = mrisr._lib
    lat = x.clone()
    t_lat, t_e = L.as_tensor(lat), L.as_tensor(torch.cat([ctx, ctx]).contiguous())
    c0 = tiny["cfg"].block_out_channels[0]
    bad = torch.zeros((4, c0, 8, 8)).cuda()
    f_arr = L.tensor_array([L.as_tensor(bad)])
    L.check(L.lib().mrisr_sampler_set_pag(one._h, 1, 2.0))
    with pytest.raises(RuntimeError, match="shape"):
        L.check(L.lib().mrisr_sampler_run_pag(one._h, C.byref(t_lat), None, None, C.byref(t_e), None, f_arr, 1, 0, 0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(run(fresh()), got[3])


# ------------------------------------------------------------------------------------------------ 4. bf16
@pytest.mark.parametrize("with_cfg", [False, True], ids=["pag", "pag+cfg"])
def test_pag_ddim_step_bf16(tiny, with_cfg):
    import mrisr
    from oracle import schedulers as osch
    cfg, B, g, s = tiny["cfg"], 2, 2.0, 1.0
    ctx_u, ctx_c = contexts(cfg, B, 2881)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(2882))
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(5)
    t0 = int(so.timesteps[0])
    kw = dict(pag_scale=s, pag_applied_layers=OUTER)
    if with_cfg:
        wrapped = PagUNet(tiny["o_unet"], ctx_c, s, OUTER, ctx_u=ctx_u.expand(B, -1, -1), guidance_scale=g)
        kw.update(uncond_hidden_states=ctx_u.cuda(), guidance_scale=g)
        bound = 5e-2 * (1 + 2 * (g - 1) + 2 * s)
    else:
        wrapped = PagUNet(tiny["o_unet"], ctx_c, s, OUTER)
        bound = 5e-2 * (1 + 2 * s)
    e_ref = wrapped(x, torch.tensor(t0)).sample
    x1_ref = so.ddim_step(e_ref, t0, x)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    smp = mrisr.Sampler(net, host_scheduler("ddim", 5), kind="ddim")
    smp.set_range(0, 1)
    lat = x.cuda().clone()
    smp.run(lat, ctx_c.cuda(), **kw)
    torch.cuda.synchronize()
    cx, ce = so.ddim_coeffs(t0)
    e_dev = (lat.double().cpu() - cx * x.double()) / ce  # the combined prediction the step consumed
    r_x, r_e = rel(lat, x1_ref), rel(e_dev, e_ref)
    moved = rel(e_ref, wrapped.last[2])
    print(f"bf16 PAG DDIM step cfg={with_cfg}: state rel {r_x:.3e}, combined eps rel {r_e:.3e} (bound {bound}); PAG moves eps by {moved:.3e}")
    assert r_x < bound and r_e < bound, (r_x, r_e)
    assert moved > 2 * bound or with_cfg  # PAG alone: the effect checked is larger than the tolerance it is checked at


# ------------------------------------------------------------------------------------------------ 5. log_validation
def test_log_validation_with_pag(tiny):
    import mrisr
    cfg, n = tiny["cfg"], 3
    gen = torch.Generator().manual_seed(2891)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(256, 256), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    _, ctx_c = contexts(cfg, 1, 2892)
    vae, acc = StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(2893)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(tiny["unet"], None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx_c.cuda(),
                                               num_inference_steps=n, **kw))

    plain = panel()
    got = panel(pag_scale=3.0, pag_applied_layers=ALL)
    W = got.shape[1] // 3
    assert not np.array_equal(plain[:, W:2 * W], got[:, W:2 * W])
    assert np.array_equal(plain[:, :W], got[:, :W]) and np.array_equal(plain[:, 2 * W:], got[:, 2 * W:])
    assert np.array_equal(plain, panel(pag_scale=0.0))
    assert np.array_equal(plain, panel(pag_scale=0.0, pag_applied_layers=ALL))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_pag_refusals_are_raised_before_any_launch(tiny):
    import mrisr
    from oracle import unet as ou
    L = mrisr._lib
    sp, x, ctx = ddim_setup(tiny, n=3)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    lat = x.clone()
    for kw, what in ((dict(pag_scale=-1.0), "pag_scale"),
                     (dict(pag_scale=float("nan")), "pag_scale"),
                     (dict(pag_scale=float("inf")), "pag_scale"),
                     (dict(pag_scale=1.0, pag_applied_layers=()), "pag_applied_layers"),
                     (dict(pag_scale=1.0, pag_applied_layers=("down_blocks.3",)), "pag_applied_layers"),
                     (dict(pag_scale=0.0, pag_applied_layers=("nope",)), "pag_applied_layers"),
                     (dict(pag_scale=1.0, guidance_rescale=1.5), "guidance_rescale"),
                     (dict(pag_scale=1.0, guidance_scale=3.0), "uncond_hidden_states")):
        with pytest.raises(ValueError, match=what):
            smp.run(lat, ctx, **kw)
    cached = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    cached.set_cache(2, 1)
    with pytest.raises(ValueError, match="cache"):
        cached.run(lat, ctx, pag_scale=1.0)
    # C*h*w of the latents not a multiple of 4: only a 1-channel UNet can be asked for that
    mcfg = ou.MNIST
    mnet = mrisr.UNet2DConditionModel(mcfg, compute_dtype="f32")
    mnet.load_state_dict(ou.init_unet_params(mcfg, seed=2211, perturb_norm=True))
    odd = torch.randn((2, 1, 3, 3)).cuda()
    keep = odd.clone()
    with pytest.raises(ValueError, match="multiple of 4"):
        mrisr.Sampler(mnet, host_scheduler("ddim", 3), kind="ddim").run(odd, torch.randn((2, 77, mcfg.cross_attention_dim)).cuda(), pag_scale=1.0)
    assert torch.equal(odd, keep)
    # a UNet built with fp8_attention
    f8 = mrisr.UNet2DConditionModel(tiny["cfg"], compute_dtype="bf16", fp8_attention=True)
    with pytest.raises(ValueError, match="fp8_attention"):
        mrisr.Sampler(f8, sp, kind="ddim").run(lat, ctx, pag_scale=1.0)
    with pytest.raises(mrisr.MrisrError, match="fp8_attention"):
        f8.set_pag(1, 0, 1)
    # the C ABI refuses by itself what it could not honour
    with pytest.raises(mrisr.MrisrError, match="ControlNet"):
        L.check(L.lib().mrisr_model_set_pag(tiny["cnet"]._h, 1, 0, 1))
    with pytest.raises(mrisr.MrisrError, match="block_mask"):
        tiny["unet"].set_pag(1 << 16, 0, 1)
    with pytest.raises(mrisr.MrisrError, match="pag_scale"):
        L.check(L.lib().mrisr_sampler_set_pag(smp._h, 1, -1.0))
    with pytest.raises(mrisr.MrisrError, match="block_mask"):
        L.check(L.lib().mrisr_sampler_set_pag(smp._h, 0, 1.0))
    with pytest.raises(mrisr.MrisrError, match="block_mask"):
        L.check(L.lib().mrisr_sampler_set_pag(smp._h, 1 << 16, 1.0))
    t_lat, t_e = L.as_tensor(lat), L.as_tensor(ctx.contiguous())
    L.check(L.lib().mrisr_sampler_set_pag(smp._h, 1 << 6, 1.0))
    with pytest.raises(mrisr.MrisrError, match="encoder_hidden_states"):  # [B] rows where 2B are needed
        L.check(L.lib().mrisr_sampler_run_pag(smp._h, C.byref(t_lat), None, None, C.byref(t_e), None, None, 0, 0, 1, L.stream_ptr()))
    L.check(L.lib().mrisr_sampler_set_cache(cached._h, 2, 1))
    L.check(L.lib().mrisr_sampler_set_pag(cached._h, 1 << 6, 1.0))
    t_e2 = L.as_tensor(torch.cat([ctx, ctx]).contiguous())
    with pytest.raises(mrisr.MrisrError, match="cache"):
        L.check(L.lib().mrisr_sampler_run_pag(cached._h, C.byref(t_lat), None, None, C.byref(t_e2), None, None, 0, 0, 1, L.stream_ptr()))
    # a forward whose batch does not hold the perturbed range; a cached forward; a training step - all while the state is set
    net = mrisr.UNet2DConditionModel(tiny["cfg"], compute_dtype="f32", lora_rank=4, lora_alpha=4, lora_fused=True)
    net.load_state_dict(tiny["p"])
    t = torch.tensor(500)
    net.set_pag(1 << 6, 1, 2)
    try:
        with pytest.raises(mrisr.MrisrError, match="outside the batch"):
            net(x, t, encoder_hidden_states=ctx)
        net.set_pag(1 << 6, 0, 1)
        cb, cc, ch, cw = net.cache_shape(1, 2, 16, 16)
        with pytest.raises(mrisr.MrisrError, match="feature cache"):
            net.forward_cached(x, t, ctx, torch.zeros((cb, ch, cw, cc), device="cuda"), 1, False)
        tr = mrisr.LoRATrainer(net)
        with pytest.raises(mrisr.MrisrError, match="perturbed-attention"):
            tr.forward_backward(x, torch.full((2,), 500, dtype=torch.int64).cuda(), ctx, torch.zeros_like(x))
    finally:
        net.set_pag()
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran on the latents
