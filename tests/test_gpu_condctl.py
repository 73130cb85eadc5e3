"""GPU: conditioning strength in the graph sampler (``Sampler.run(controlnet_conditioning_scale=,
control_guidance_start=, control_guidance_end=, adapter_conditioning_scale=, adapter_conditioning_factor=, guess_mode=, conditioning=)``).
TINY UNet and ControlNet, f32 engine, 5 steps, latents [2, 4, 16, 16] unless stated.

* the constant table {1, 1} is the run without the keywords, bit for bit: fma(1, r, x) is the add of before, and the ControlNet's
  output convolutions write the same numbers to another place;
* trajectories against the CPU oracle wrapped by tests/condctl_ref.py (itself checked by test_condctl_cpu.py) at 1e-3 relative L2 and
  max-relative - the f32 tolerance of every sampler test here.  Each first asserts ON THE ORACLE that its reference ends at least ten
  times that tolerance away from the reference at full strength, so a device run that ignored the table could not pass;
* c = 0 on every step against a sampler built without the ControlNet at 1e-3 (in exact arithmetic the two are identical);
* graph == eager; other values replay the stored graph; switching guess mode or clearing the table captures again;
* one bf16 step at 3 x 5e-2, test_gpu_guidance.py's convention; ``log_validation``; every refusal, before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import condctl_ref as cr
import freeu_ref as fr
from guidance_ref import GuidedControlNet, GuidedUNet
from pag_ref import CtxControlNet, PagUNet
from pag_testlib import StubVAE, maxrel, rel
from schedule_ref import ScheduledUNet
from tiles_ref import TiledControlNet, TiledUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N = 5
TOL = 1e-3
OUTER = ("down_blocks.0", "up_blocks.3")


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=4201, perturb_norm=True)
    cp = ou.init_controlnet_params(cfg, seed=4202, perturb_norm=True)
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32")
    unet.load_state_dict(p)
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="f32")
    cnet.load_state_dict(cp)
    return dict(cfg=cfg, p=p, cp=cp, unet=unet, cnet=cnet, o_unet=ou.OracleUNet(p, cfg), o_cnet=ou.OracleControlNet(cp, cfg))


def setup(cfg, seed, B=2, hw=16, n=N):
    """x, LR anchor, step noise [n, B, ...], uncond context [1, L, D], cond context [B, L, D], condition image, adapter features."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, hw, hw), generator=g)
    lr = 0.18215 * torch.randn((B, 4, hw, hw), generator=g)
    z = torch.randn((n, B, 4, hw, hw), generator=g)
    cu = torch.randn((1, 77, cfg.cross_attention_dim), generator=g)
    cc = torch.randn((B, 77, cfg.cross_attention_dim), generator=g)
    cond = torch.randn((B, 3, 8 * hw, 8 * hw), generator=g)
    feats = [torch.randn((B, c, hw >> i, hw >> i), generator=g) for i, c in enumerate(cfg.block_out_channels)]
    return dict(x=x, lr=lr, z=z, cu=cu, cc=cc, cond=cond, feats=feats)


def host_scheduler(kind, n=N):
    import mrisr
    cls = {"ddim": mrisr.DDIMScheduler, "resshift": mrisr.DDPMScheduler, "unipc": mrisr.UniPCMultistepScheduler,
           "dpmsolver++": mrisr.DPMSolverMultistepScheduler}[kind]
    sp = cls(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    return sp


def oracle_scheduler(n=N):
    from oracle import schedulers as osch
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    return so


def captures(smp):
    import mrisr
    return int(mrisr._lib.lib().mrisr_sampler_num_captures(smp._h))


def run(smp, x0, ctx, **kw):
    """One run from x0 on this sampler's own latents buffer (the latents' address is part of the graph key)."""
    if getattr(smp, "_test_latents", None) is None or smp._test_latents.shape != x0.shape:
        smp._test_latents = torch.empty_like(x0).contiguous()
    lat = smp._test_latents
    lat.copy_(x0)
    smp.run(lat, ctx, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


def guard(tag, ref_final, full_final):
    """The effect-size guard, on the oracle alone: the reference differs from the one at full strength by >= 10 x the tolerance."""
    d = rel(ref_final, full_final)
    print(f"{tag}: oracle reference vs full strength: rel {d:.3e} (needs >= {10 * TOL:.0e})")
    assert d >= 10 * TOL, (tag, d)


def check_states(tag, make_sampler, x0, traj, n, run_kw):
    """Every state of an n-step run (set_range stops the fused loop after k steps) against the oracle's."""
    smp = make_sampler()
    for k in range(1, n + 1):
        lat = x0.clone().contiguous()
        smp.set_range(0, k)
        smp.run(lat, **run_kw)
        torch.cuda.synchronize()
        r, m = rel(lat, traj[k]), maxrel(lat, traj[k])
        print(f"{tag}: state {k}/{n} rel {r:.3e} maxrel {m:.3e}")
        assert r < TOL and m < TOL, (tag, k, r, m)


# ------------------------------------------------------------------------------------------------ 1. the constant table is the run of before
def test_neutral_table_is_the_run_without_it_ddim_controlnet(tiny):
    import mrisr
    s = setup(tiny["cfg"], 4301)
    sp = host_scheduler("ddim")
    kw = dict(controlnet_cond=s["cond"].cuda())
    a = run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), s["cc"].cuda(), **kw)
    smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    b = run(smp, s["x"].cuda(), s["cc"].cuda(), conditioning=cr.constant_rows(N), **kw)
    assert torch.equal(a, b) and not torch.equal(a, s["x"]) and captures(smp) == 1
    # the keywords at their defaults build no table at all
    c = run(smp, s["x"].cuda(), s["cc"].cuda(), controlnet_conditioning_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0,
            adapter_conditioning_scale=1.0, adapter_conditioning_factor=1.0, guess_mode=False, **kw)
    assert torch.equal(a, c) and captures(smp) == 2
    # the state is gone from the handles: plain forwards add at full strength, through the path of before
    t = torch.tensor(500)
    down, mid = tiny["cnet"](s["x"].cuda(), t, encoder_hidden_states=s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), return_dict=False)
    e = tiny["unet"](s["x"].cuda(), t, encoder_hidden_states=s["cc"].cuda(), down_block_additional_residuals=down,
                     mid_block_additional_residual=mid).sample.cpu()
    d_o, m_o = tiny["o_cnet"](s["x"], t, encoder_hidden_states=s["cc"], controlnet_cond=s["cond"], return_dict=False)
    ref = tiny["o_unet"](s["x"], t, encoder_hidden_states=s["cc"], down_block_additional_residuals=d_o, mid_block_additional_residual=m_o).sample
    assert rel(e, ref) < TOL


def test_neutral_table_is_the_run_without_it_resshift_noise_cfg(tiny):
    import mrisr
    s = setup(tiny["cfg"], 4302)
    sp = host_scheduler("resshift")
    lr = s["lr"].cuda()
    x0 = mrisr.get_res_shifting_latents(lr, lr, sp.timesteps[0], sp, s["z"][0].cuda())
    kw = dict(lr_latents=lr, step_noise=s["z"][:N - 1].cuda(), controlnet_cond=s["cond"].cuda(), uncond_hidden_states=s["cu"].cuda(),
              guidance_scale=3.0, guidance_rescale=0.7)
    a = run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift"), x0, s["cc"].cuda(), **kw)
    b = run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="resshift"), x0, s["cc"].cuda(), conditioning=cr.constant_rows(N), **kw)
    assert torch.equal(a, b) and not torch.equal(a, x0.cpu())


def test_neutral_table_is_the_run_without_it_unipc_adapter(tiny):
    import mrisr
    s = setup(tiny["cfg"], 4303)
    sp = host_scheduler("unipc")
    kw = dict(adapter_features=[f.cuda() for f in s["feats"]])
    a = run(mrisr.Sampler(tiny["unet"], sp, kind="unipc"), s["x"].cuda(), s["cc"].cuda(), **kw)
    b = run(mrisr.Sampler(tiny["unet"], sp, kind="unipc"), s["x"].cuda(), s["cc"].cuda(), conditioning=cr.constant_rows(N), **kw)
    assert torch.equal(a, b) and not torch.equal(a, s["x"])


# ------------------------------------------------------------------------------------------------ 2. against condctl_ref on the CPU oracle
def ddim_controlnet_case(tiny, tag, seed, rows, run_kw, guess=False):
    """DDIM with the ControlNet, unguided: oracle trajectory with `rows`, the guard against full strength, then every device state."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], seed)

    def oracle(r, g):
        return osa.ddim_sample(tiny["o_unet"], s["x"], s["cc"], oracle_scheduler(), cr.ScaledControlNet(tiny["o_cnet"], r, guess=g), s["cond"])
    traj = oracle(rows, guess)
    guard(tag, traj[N], oracle(cr.constant_rows(N), False)[N])
    sp = host_scheduler("ddim")
    kw = dict(encoder_hidden_states=s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), **run_kw)
    check_states(tag, lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)


def test_controlnet_conditioning_scale(tiny):
    ddim_controlnet_case(tiny, "controlnet scale 0.5", 4311, cr.table(N, 0.5), dict(controlnet_conditioning_scale=0.5))


def test_control_guidance_interval(tiny):
    rows = cr.table(N, 1.0, 0.2, 0.8)
    assert rows[:, 0].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    ddim_controlnet_case(tiny, "control guidance (0.2, 0.8)", 4312, rows, dict(control_guidance_start=0.2, control_guidance_end=0.8))


def test_guess_mode_unguided(tiny):
    ddim_controlnet_case(tiny, "guess mode, unguided", 4313, cr.constant_rows(N), dict(guess_mode=True), guess=True)


def test_adapter_conditioning_scale_and_factor(tiny):
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 4314)
    rows = cr.table(N, a=0.6, factor=0.6)
    assert rows[:, 1].tolist() == [np.float32(0.6)] * 3 + [0.0, 0.0]

    def oracle(r):
        return osa.ddim_sample(cr.ScaledAdapterUNet(tiny["o_unet"], r), s["x"], s["cc"], oracle_scheduler(), intrablock=[f.clone() for f in s["feats"]])
    traj = oracle(rows)
    guard("adapter 0.6 x 0.6", traj[N], oracle(cr.constant_rows(N))[N])
    sp = host_scheduler("ddim")
    kw = dict(encoder_hidden_states=s["cc"].cuda(), adapter_features=[f.cuda() for f in s["feats"]], adapter_conditioning_scale=0.6,
              adapter_conditioning_factor=0.6)
    check_states("adapter 0.6 x 0.6", lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim"), s["x"].cuda(), traj, N, kw)


def test_controlnet_scale_with_cfg_and_rescale(tiny):
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 4315)
    g, phi, cu = 3.0, 0.7, s["cu"].expand(2, -1, -1)
    rows = cr.table(N, 0.5, 0.0, 0.8)

    def oracle(r):
        return osa.ddim_sample(GuidedUNet(tiny["o_unet"], cu, s["cc"], g, phi), s["x"], None, oracle_scheduler(),
                               cr.ScaledControlNet(GuidedControlNet(tiny["o_cnet"], cu, s["cc"]), r), s["cond"])
    traj = oracle(rows)
    guard("controlnet scale + cfg", traj[N], oracle(cr.constant_rows(N))[N])
    sp = host_scheduler("ddim")
    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, guidance_rescale=phi,
              controlnet_cond=s["cond"].cuda(), controlnet_conditioning_scale=0.5, control_guidance_end=0.8)
    check_states("controlnet scale + cfg", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)


def test_controlnet_scale_with_pag_alone(tiny):
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 4316)
    ps = 2.0
    rows = cr.table(N, 0.5)

    def oracle(r):
        return osa.ddim_sample(PagUNet(tiny["o_unet"], s["cc"], ps, OUTER), s["x"], None, oracle_scheduler(),
                               cr.ScaledControlNet(CtxControlNet(tiny["o_cnet"], s["cc"]), r), s["cond"])
    traj = oracle(rows)
    guard("controlnet scale + pag", traj[N], oracle(cr.constant_rows(N))[N])
    sp = host_scheduler("ddim")
    kw = dict(encoder_hidden_states=s["cc"].cuda(), pag_scale=ps, pag_applied_layers=OUTER, controlnet_cond=s["cond"].cuda(),
              controlnet_conditioning_scale=0.5)
    check_states("controlnet scale + pag", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)


def test_dpmsolver_with_lr_latents(tiny):
    import mrisr
    import multistep_ref as mref
    s = setup(tiny["cfg"], 4317)
    sp = host_scheduler("dpmsolver++")
    rows = cr.table(N, 0.5, 0.2, 1.0)

    def oracle(r):
        return mref.multistep_sample("dpmsolver++", tiny["o_unet"], s["x"], s["cc"], sp.timesteps, sp.alphas_cumprod, lr_latents=s["lr"],
                                     controlnet=cr.ScaledControlNet(tiny["o_cnet"], r), control_image=s["cond"], last=N)
    traj = oracle(rows)
    guard("dpmsolver++ + lr + controlnet scale", traj[N], oracle(cr.constant_rows(N))[N])
    kw = dict(encoder_hidden_states=s["cc"].cuda(), lr_latents=s["lr"].cuda(), controlnet_cond=s["cond"].cuda(),
              controlnet_conditioning_scale=0.5, control_guidance_start=0.2)
    check_states("dpmsolver++ + lr + controlnet scale", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="dpmsolver++"),
                 s["x"].cuda(), traj, N, kw)


def test_controlnet_scale_with_tiles(tiny):
    """16 x 16 canvas, tile 8, overlap 0 (T = 4), 3 steps: the ControlNet and the scaled adds run on the tile batch."""
    import mrisr
    from oracle import sampler as osa
    n = 3
    s = setup(tiny["cfg"], 4318, n=n)
    rows = cr.table(n, 0.5, 0.0, 0.7)
    assert rows[:, 0].tolist() == [0.5, 0.5, 0.0]

    def oracle(r):
        return osa.ddim_sample(TiledUNet(tiny["o_unet"], 16, 16, 8, 0), s["x"], s["cc"], oracle_scheduler(n),
                               cr.ScaledControlNet(TiledControlNet(tiny["o_cnet"], 16, 16, 8, 0), r), s["cond"])
    traj = oracle(rows)
    guard("controlnet scale + tiles", traj[n], oracle(cr.constant_rows(n))[n])
    sp = host_scheduler("ddim", n)

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
        smp.set_tiles(8, 0)
        return smp
    kw = dict(encoder_hidden_states=s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), controlnet_conditioning_scale=0.5, control_guidance_end=0.7)
    check_states("controlnet scale + tiles", make, s["x"].cuda(), traj, n, kw)


def test_set_range_reads_the_rows_of_its_steps(tiny):
    """set_range(2, 5) with five distinct rows: steps 2..4 read rows 2..4 (an absolute index, like the coefficient rows)."""
    import mrisr
    s = setup(tiny["cfg"], 4319)
    so = oracle_scheduler()
    rows = cr.constant_rows(N)
    rows[:, 0] = (9.0, 7.0, 0.5, 0.0, 1.5)

    def oracle(r):
        wc = cr.ScaledControlNet(tiny["o_cnet"], r, first=2)
        x = s["x"]
        for t in so.timesteps.tolist()[2:]:
            tt = torch.tensor(t, dtype=torch.int64)
            d, m = wc(x, tt, encoder_hidden_states=s["cc"], controlnet_cond=s["cond"])
            x = so.ddim_step(tiny["o_unet"](x, tt, encoder_hidden_states=s["cc"], down_block_additional_residuals=d,
                                            mid_block_additional_residual=m).sample, t, x)
        assert wc.used == [float(v) for v in r[2:, 0]]
        return x
    ref = oracle(rows)
    guard("set_range(2, 5)", ref, oracle(cr.constant_rows(N)))
    smp = mrisr.Sampler(tiny["unet"], host_scheduler("ddim"), tiny["cnet"], kind="ddim")
    smp.set_range(2, 5)
    lat = run(smp, s["x"].cuda(), s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), conditioning=rows)
    r, m = rel(lat, ref), maxrel(lat, ref)
    print(f"set_range(2, 5) with a conditioning table: rel {r:.3e} maxrel {m:.3e}")
    assert r < TOL and m < TOL
    shifted = np.roll(rows, 2, axis=0)  # rows 0..2 of this table are rows 3, 4, 0 of the other: a relative index would read these
    assert rel(run(smp, s["x"].cuda(), s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), conditioning=shifted), ref) > 10 * TOL


def test_schedule_and_conditioning_table_in_one_run(tiny):
    """A FreeU interval from the [n, 8] schedule table and a ControlNet interval from the conditioning table, both read behind one step
    counter."""
    import mrisr
    from oracle import sampler as osa
    cfg, unet = tiny["cfg"], tiny["unet"]
    s = setup(cfg, 4320)
    sp = host_scheduler("ddim")
    rows8 = mrisr.step_schedule(sp.timesteps, freeu=fr.SD15_DOCS, freeu_interval=(0.0, 0.6))
    rows4 = cr.table(N, 0.5, 0.2, 1.0)

    def oracle(r):
        return osa.ddim_sample(ScheduledUNet(tiny["o_unet"], rows8, "plain", s["cc"], freeu=True, cfg=cfg), s["x"], s["cc"], oracle_scheduler(),
                               cr.ScaledControlNet(tiny["o_cnet"], r), s["cond"])
    traj = oracle(rows4)
    guard("schedule + conditioning", traj[N], oracle(cr.constant_rows(N))[N])
    kw = dict(encoder_hidden_states=s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), freeu_interval=(0.0, 0.6),
              controlnet_conditioning_scale=0.5, control_guidance_start=0.2)
    unet.enable_freeu(*fr.SD15_DOCS)
    try:
        check_states("schedule + conditioning", lambda: mrisr.Sampler(unet, sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)
    finally:
        unet.disable_freeu()


def test_guess_mode_under_cfg(tiny):
    """The ControlNet on the B conditional rows only; the unconditional rows of the UNet's batch get no residual."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 4321)
    g, cu = 3.0, s["cu"].expand(2, -1, -1)
    rows = cr.table(N, 0.8)

    def oracle(r, guess):
        wc = cr.ScaledControlNet(tiny["o_cnet"], r, guess=True, ctx_c=s["cc"]) if guess else \
            cr.ScaledControlNet(GuidedControlNet(tiny["o_cnet"], cu, s["cc"]), r)
        return osa.ddim_sample(GuidedUNet(tiny["o_unet"], cu, s["cc"], g), s["x"], None, oracle_scheduler(), wc, s["cond"])
    traj = oracle(rows, True)
    guard("guess mode + cfg", traj[N], oracle(cr.constant_rows(N), False)[N])
    sp = host_scheduler("ddim")
    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, controlnet_cond=s["cond"].cuda(),
              controlnet_conditioning_scale=0.8, guess_mode=True)
    check_states("guess mode + cfg", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)


# ------------------------------------------------------------------------------------------------ 3. scale 0
def test_scale_zero_is_the_sampler_without_a_controlnet(tiny):
    """In exact arithmetic identical; on the device fma(0, r, x) == x for finite r, so the bits agree too (measured: rel 0.0)."""
    import mrisr
    s = setup(tiny["cfg"], 4331)
    sp = host_scheduler("ddim")
    a = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), s["x"].cuda(), s["cc"].cuda())
    b = run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), s["cc"].cuda(), controlnet_cond=s["cond"].cuda(),
            controlnet_conditioning_scale=0.0)
    full = run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), s["cc"].cuda(), controlnet_cond=s["cond"].cuda())
    r, m = rel(b, a), maxrel(b, a)
    print(f"c = 0 vs no ControlNet: rel {r:.3e} maxrel {m:.3e}; full strength is {rel(full, a):.3e} away")
    assert r < TOL and m < TOL and rel(full, a) >= 10 * TOL


# ------------------------------------------------------------------------------------------------ 4. the sampler's state
def test_graph_replay_equals_eager_launches(tiny):
    import mrisr
    s = setup(tiny["cfg"], 4341)
    sp = host_scheduler("ddim")
    kw = dict(uncond_hidden_states=s["cu"].cuda(), guidance_scale=3.0, controlnet_cond=s["cond"].cuda(),
              adapter_features=[f.cuda() for f in s["feats"]], controlnet_conditioning_scale=0.5, control_guidance_end=0.8,
              adapter_conditioning_scale=0.6, adapter_conditioning_factor=0.6)
    for extra in (dict(), dict(guess_mode=True)):
        finals = {}
        for use_graph in (True, False):
            smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
            finals[use_graph] = run(smp, s["x"].cuda(), s["cc"].cuda(), use_graph=use_graph, **kw, **extra)
            assert captures(smp) == (1 if use_graph else 0)
        assert torch.equal(finals[True], finals[False]) and not torch.equal(finals[True], s["x"])


def test_other_values_replay_the_graph_guess_mode_and_clearing_capture_again(tiny):
    import mrisr
    s = setup(tiny["cfg"], 4342)
    sp = host_scheduler("ddim")
    smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    x, cc, kw = s["x"].cuda(), s["cc"].cuda(), dict(controlnet_cond=s["cond"].cuda())
    fresh = lambda **k: run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), x, cc, **kw, **k)  # noqa: E731
    ta, tb = cr.table(N, 0.5, 0.2, 0.8), cr.table(N, 1.5, 0.0, 0.6)
    a = run(smp, x, cc, conditioning=ta, **kw)
    assert captures(smp) == 1
    b = run(smp, x, cc, conditioning=tb, **kw)
    assert captures(smp) == 1 and not torch.equal(a, b)                      # other values, equal flags: the stored graph
    assert torch.equal(run(smp, x, cc, conditioning=ta, **kw), a) and captures(smp) == 1
    assert torch.equal(b, fresh(conditioning=tb))                            # nothing stale
    c = run(smp, x, cc, conditioning=ta, guess_mode=True, **kw)              # guess mode: other weights, another graph
    assert captures(smp) == 2 and not torch.equal(c, a) and torch.equal(c, fresh(conditioning=ta, guess_mode=True))
    d = run(smp, x, cc, **kw)                                                # cleared: the adds of before
    assert captures(smp) == 3 and torch.equal(d, fresh())
    assert torch.equal(run(smp, x, cc, conditioning=ta, **kw), a) and captures(smp) == 4


# ------------------------------------------------------------------------------------------------ 5. bf16, log_validation, refusals
def test_scaled_ddim_step_bf16(tiny):
    """Step 1 of 5 alone (set_range(1, 2)) on a table whose row 1 has c = 0.5, bf16 UNet and ControlNet, against the oracle's step at
    3 x 5e-2 (test_gpu_guidance.py's convention for a bf16 step that combines forwards)."""
    import mrisr
    cfg = tiny["cfg"]
    s = setup(cfg, 4351)
    so = oracle_scheduler()
    rows = cr.constant_rows(N)
    rows[1, 0] = 0.5
    t1 = int(so.timesteps[1])
    tt = torch.tensor(t1)
    d, m = cr.ScaledControlNet(tiny["o_cnet"], rows, first=1)(s["x"], tt, encoder_hidden_states=s["cc"], controlnet_cond=s["cond"])
    e_ref = tiny["o_unet"](s["x"], tt, encoder_hidden_states=s["cc"], down_block_additional_residuals=d, mid_block_additional_residual=m).sample
    x_ref = so.ddim_step(e_ref, t1, s["x"])
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    unet.load_state_dict(tiny["p"])
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="bf16")
    cnet.load_state_dict(tiny["cp"])
    smp = mrisr.Sampler(unet, host_scheduler("ddim"), cnet, kind="ddim")
    smp.set_range(1, 2)
    lat = run(smp, s["x"].cuda(), s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), conditioning=rows)
    cx, ce = so.ddim_coeffs(t1)
    e_dev = (lat.double() - cx * s["x"].double()) / ce
    r_x, r_e = rel(lat, x_ref), rel(e_dev, e_ref)
    print(f"bf16 DDIM step, row 1 (c = 0.5): state rel {r_x:.3e}, eps rel {r_e:.3e} (bound {3 * 5e-2})")
    assert r_x < 3 * 5e-2 and r_e < 3 * 5e-2, (r_x, r_e)


def test_log_validation_keywords(tiny):
    import mrisr
    cfg, n = tiny["cfg"], 3
    gen = torch.Generator().manual_seed(4361)
    base = torch.randn((1, 1, 32, 32), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(512, 512), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    ctx = torch.randn((1, 77, cfg.cross_attention_dim), generator=gen).cuda()
    vae, acc = StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(4362)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(tiny["unet"], tiny["cnet"], vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx,
                                               num_inference_steps=n, **kw))
    plain = panel()
    W = plain.shape[1] // 3
    assert np.array_equal(plain, panel(controlnet_conditioning_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0,
                                       adapter_conditioning_scale=1.0, adapter_conditioning_factor=1.0, guess_mode=False))
    half = panel(controlnet_conditioning_scale=0.5)
    guess = panel(guess_mode=True)
    late = panel(control_guidance_start=0.4)
    for p in (half, guess, late):
        assert not np.array_equal(p[:, W:2 * W], plain[:, W:2 * W]) and np.array_equal(p[:, :W], plain[:, :W]) and np.array_equal(p[:, 2 * W:], plain[:, 2 * W:])
    assert not np.array_equal(half, guess) and np.array_equal(plain, panel())
    with pytest.raises(ValueError, match="adapter_features"):
        panel(adapter_conditioning_scale=0.5)


def test_refusals_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    s = setup(tiny["cfg"], 4371)
    x, cc, cu, cond = s["x"].cuda(), s["cc"].cuda(), s["cu"].cuda(), s["cond"].cuda()
    feats = [f.cuda() for f in s["feats"]]
    lat = x.clone()
    sp = host_scheduler("ddim")
    with_c = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    no_c = mrisr.Sampler(tiny["unet"], sp, kind="ddim")

    def set_table(smp, rows, n=None, guess=0):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        L.check(L.lib().mrisr_sampler_set_conditioning(smp._h, rows.ctypes.data_as(C.c_void_p), len(rows) if n is None else n, guess))

    # ---- mrisr_sampler_set_conditioning, before any device work, naming row and field
    bad = cr.constant_rows(N)
    with pytest.raises(mrisr.MrisrError, match="n_steps"):
        set_table(with_c, bad[:4])
    for (i, c, v), word in (((3, 0, np.nan), r"row 3: controlnet scale \(c\) is not finite"), ((1, 1, np.inf), r"row 1: adapter scale \(a\) is not finite"),
                            ((2, 2, 0.5), "row 2: column 2 must be 0"), ((4, 3, -1.0), "row 4: column 3 must be 0")):
        t = bad.copy()
        t[i, c] = v
        with pytest.raises(mrisr.MrisrError, match=word):
            set_table(with_c, t)
    with pytest.raises(mrisr.MrisrError, match="clears"):
        set_table(with_c, bad, n=0)
    # ---- Python, on numbers alone
    for kw, word in ((dict(conditioning=bad[:4]), "shape"), (dict(conditioning=bad, controlnet_conditioning_scale=0.5), "excludes"),
                     (dict(controlnet_conditioning_scale=float("nan")), "finite"), (dict(control_guidance_start=0.9, control_guidance_end=0.1), "start"),
                     (dict(adapter_conditioning_scale=0.5), "adapter_features"), (dict(guess_mode=True, pag_scale=2.0), "guess_mode"),
                     (dict(adapter_conditioning_factor=2.0, adapter_features=feats), "factor")):
        with pytest.raises(ValueError, match=word):
            with_c.run(lat, cc, controlnet_cond=cond, **kw)
    for kw in (dict(controlnet_conditioning_scale=0.5), dict(guess_mode=True), dict(control_guidance_end=0.5)):
        with pytest.raises(ValueError, match="ControlNet"):
            no_c.run(lat, cc, **kw)
    tiled = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    tiled.set_tiles(8, 0)
    with pytest.raises(ValueError, match="tiles"):
        tiled.run(lat, cc, controlnet_cond=cond, guess_mode=True)
    cached = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    cached.set_cache(2, 1)
    with pytest.raises(ValueError, match="cache"):
        cached.run(lat, cc, adapter_features=feats, adapter_conditioning_scale=0.5)
    # none of the refused calls left a table behind: the next run without the keywords is the plain run
    fresh_c = run(mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), x, cc, controlnet_cond=cond)
    fresh_n = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x, cc)
    assert torch.equal(run(with_c, x, cc, controlnet_cond=cond), fresh_c) and torch.equal(run(no_c, x, cc), fresh_n)
    # ---- the C ABI's own run-time rules, with a table set by hand
    t_lat, t_e, t_e2 = L.as_tensor(lat), L.as_tensor(cc), L.as_tensor(torch.cat([cc, cc]).contiguous())
    t_c, t_c2 = L.as_tensor(cond), L.as_tensor(torch.cat([cond, cond]).contiguous())
    f_arr = L.tensor_array([L.as_tensor(f) for f in feats])

    def c_run(smp, cond_t=None, n_feats=0):
        L.check(L.lib().mrisr_sampler_run(smp._h, C.byref(t_lat), None, None, C.byref(t_e), C.byref(cond_t) if cond_t else None,
                                          f_arr if n_feats else None, n_feats, 1, L.stream_ptr()))
    half_c, half_a = cr.constant_rows(N, c=0.5), cr.constant_rows(N, a=0.5)
    set_table(no_c, half_c)
    with pytest.raises(mrisr.MrisrError, match=r"controlnet scale \(c\) != 1 need a sampler with a ControlNet"):
        c_run(no_c)
    set_table(no_c, bad, guess=1)
    with pytest.raises(mrisr.MrisrError, match="guess mode needs a sampler with a ControlNet"):
        c_run(no_c)
    set_table(no_c, half_a)
    with pytest.raises(mrisr.MrisrError, match=r"adapter scale \(a\) != 1 need a run with adapter features"):
        c_run(no_c)
    set_table(with_c, half_a)
    with pytest.raises(mrisr.MrisrError, match=r"adapter scale \(a\) != 1 need a run with adapter features"):
        c_run(with_c, t_c)
    set_table(with_c, half_c, guess=1)
    L.check(L.lib().mrisr_sampler_set_pag(with_c._h, 1 << 6, 2.0))
    with pytest.raises(mrisr.MrisrError, match="guess mode in a pag run is not supported"):
        L.check(L.lib().mrisr_sampler_run_pag(with_c._h, C.byref(t_lat), None, None, C.byref(t_e2), C.byref(t_c2), None, 0, 0, 1, L.stream_ptr()))
    set_table(tiled, half_c, guess=1)
    with pytest.raises(mrisr.MrisrError, match="guess mode together with tiles is not supported"):
        c_run(tiled, t_c)
    set_table(cached, half_a)
    with pytest.raises(mrisr.MrisrError, match="conditioning table together with a feature cache"):
        c_run(cached, None, len(feats))
    # guess mode under guidance takes the condition image at [B]: the [2B] form is refused
    set_table(with_c, half_c, guess=1)
    with pytest.raises(mrisr.MrisrError, match="guess mode: controlnet_cond must be"):
        L.check(L.lib().mrisr_sampler_run_guided(with_c._h, C.byref(t_lat), None, None, C.byref(t_e2), C.byref(t_c2), None, 0, 1, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran on the latents
    # NULL / 0 clears a table: the runs of before
    for smp in (with_c, no_c):
        L.check(L.lib().mrisr_sampler_set_conditioning(smp._h, None, 0, 0))
    assert torch.equal(run(with_c, x, cc, controlnet_cond=cond), fresh_c) and torch.equal(run(no_c, x, cc), fresh_n)
