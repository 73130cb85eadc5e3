"""GPU: ``Sampler.run(skip_neutral=True)`` - each step runs only the rows and networks its table rows need.  TINY UNet
(+ rank-4 LoRA) and ControlNet, f32 engine, 5 steps ("leading" spacing, ``steps_offset=1``), latents [2, 4, 16, 16] unless stated.

A neutral row's guided prediction IS the conditional one in exact arithmetic, so the oracles of tests/schedule_ref.py, tests/condctl_ref.py
and tests/tiles_ref.py give the expected trajectories as they stand; the tolerance is the suite's f32 sampler tolerance, 1e-3 relative
L2 and max-relative per state.  What a run did is asserted on ``Sampler.last_run_stats`` - rows, ControlNet steps, feature steps,
variants, captures - never on a timing."""
import pytest
import torch

import condctl_ref as cr
import freeu_ref as fr
from guidance_ref import GuidedControlNet
from pag_testlib import maxrel, rel
from schedule_ref import NEUTRAL, ScheduledUNet, constant_rows
from tiles_ref import TiledUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N, B, TOL = 5, 2, 1e-3
OUTER = ("down_blocks.0", "up_blocks.3")


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    from oracle import unet as ou
    cfg, p = fr.tiny_params()
    cp = ou.init_controlnet_params(cfg, seed=4202, perturb_norm=True)
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    unet.load_state_dict(p)
    cnet = mrisr.ControlNetModel(cfg, compute_dtype="f32")
    cnet.load_state_dict(cp)
    return dict(cfg=cfg, p=p, cp=cp, unet=unet, cnet=cnet, o_unet=ou.OracleUNet(p, cfg), o_cnet=ou.OracleControlNet(cp, cfg))


def setup(cfg, seed, rows=B, hw=16, n=N):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, 4, hw, hw), generator=g)
    lr = 0.18215 * torch.randn((rows, 4, hw, hw), generator=g)
    z = torch.randn((n, rows, 4, hw, hw), generator=g)
    cu = torch.randn((1, 77, cfg.cross_attention_dim), generator=g)
    cc = torch.randn((rows, 77, cfg.cross_attention_dim), generator=g)
    cond = torch.randn((rows, 3, 8 * hw, 8 * hw), generator=g)
    feats = [torch.randn((rows, c, hw >> i, hw >> i), generator=g) for i, c in enumerate(cfg.block_out_channels)]
    return dict(x=x, lr=lr, z=z, cu=cu, cc=cc, cond=cond, feats=feats)


def host_scheduler(kind, n=N):
    import mrisr
    cls = {"ddim": mrisr.DDIMScheduler, "resshift": mrisr.DDPMScheduler, "unipc": mrisr.UniPCMultistepScheduler}[kind]
    sp = cls(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(n)
    return sp


def oracle_scheduler(n=N):
    from oracle import schedulers as osch
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    return so


def run(smp, x0, ctx, **kw):
    """One run from x0 on this sampler's own latents buffer (the latents' address is part of the graph key)."""
    if getattr(smp, "_test_latents", None) is None or smp._test_latents.shape != x0.shape:
        smp._test_latents = torch.empty_like(x0).contiguous()
    lat = smp._test_latents
    lat.copy_(x0)
    smp.run(lat, ctx, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


def check_states(tag, make, x0, traj, n, run_kw):
    """Every state of an n-step run (set_range stops the fused loop after k steps) against the oracle's.  Then the whole run once more on a
    fresh sampler, whose stats and capture count the caller asserts (a growing range reallocates the per-run time-embedding table, which
    is part of the step plan: the range runs capture more often than one run does)."""
    kw = dict(run_kw)
    ctx = kw.pop("encoder_hidden_states")
    smp = make()
    for k in range(1, n + 1):
        smp.set_range(0, k)
        lat = run(smp, x0, ctx, **kw)
        r, m = rel(lat, traj[k]), maxrel(lat, traj[k])
        print(f"{tag}: state {k}/{n} rel {r:.3e} maxrel {m:.3e}")
        assert r < TOL and m < TOL, (tag, k, r, m)
    fresh = make()
    assert torch.equal(run(fresh, x0, ctx, **kw), lat)
    return fresh


def stats(smp, **want):
    got = smp.last_run_stats
    print("last_run_stats:", got)
    assert {k: got[k] for k in want} == want, (got, want)


class PairUNet:
    """Plumbing for the oracle loops, no arithmetic: hands the oracle UNet the half of a ((down_u, down_c), (mid_u, mid_c)) residual pair
    (guidance_ref.GuidedControlNet, condctl_ref.ScaledControlNet in guess mode) that belongs to the context it is called with."""

    def __init__(self, unet, ctx_u, ctx_c):
        self.unet, self.ctx_u, self.ctx_c = unet, ctx_u, ctx_c

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, **kw):
        down, mid = down_block_additional_residuals, mid_block_additional_residual
        if down is not None:
            k = 0 if encoder_hidden_states is self.ctx_u else 1
            assert encoder_hidden_states is (self.ctx_u, self.ctx_c)[k]
            kw.update(down_block_additional_residuals=down[k], mid_block_additional_residual=mid[k])
        return self.unet(sample, timestep, encoder_hidden_states=encoder_hidden_states, **kw)


# ------------------------------------------------------------------------------------------------ 1, 2. the row-window forward
@pytest.mark.parametrize("lo,hi", [(2, 4), (1, 2)])
def test_unet_row_window(tiny, lo, hi):
    """A UNet planned at 4 rows: rows [lo, hi) through the window entry against the oracle on those rows (test_gpu_unet.py's f32 bound,
    1e-3), with adapter features at the window's rows; a full-batch forward afterwards is bit-equal to the one before."""
    import mrisr
    s = setup(tiny["cfg"], 5101, rows=4)
    unet, t = tiny["unet"], torch.tensor(500)
    x, cc, feats = s["x"].cuda(), s["cc"].cuda(), [f.cuda() for f in s["feats"]]
    before = unet(x, t, encoder_hidden_states=cc, down_intrablock_additional_residuals=feats).sample.clone()
    win = unet(x[lo:hi], t, rows=(lo, hi), down_intrablock_additional_residuals=[f[lo:hi] for f in feats]).sample.cpu()
    ref = tiny["o_unet"](s["x"][lo:hi], t, encoder_hidden_states=s["cc"][lo:hi],
                         down_intrablock_additional_residuals=[f[lo:hi].clone() for f in s["feats"]]).sample
    r, m = rel(win, ref), maxrel(win, ref)
    print(f"unet rows [{lo}, {hi}) of 4: rel {r:.3e} maxrel {m:.3e}")
    assert r < 1e-3 and m < 1e-3
    other = tiny["o_unet"](s["x"][lo:hi], t, encoder_hidden_states=s["cc"][0:hi - lo],
                           down_intrablock_additional_residuals=[f[lo:hi].clone() for f in s["feats"]]).sample
    assert rel(other, ref) > 1e-2  # on the oracle: the context of rows [0, hi - lo) - caches read at row 0 - gives something else
    after = unet(x, t, down_intrablock_additional_residuals=feats).sample  # the cached context: nothing re-planned, nothing clobbered
    assert torch.equal(before, after)
    with pytest.raises(mrisr.MrisrError, match="inside the planned batch"):
        unet(x[0:2], t, rows=(3, 5))
    with pytest.raises(ValueError, match="cached for the full batch"):
        unet(x[lo:hi], t, encoder_hidden_states=cc[lo:hi], rows=(lo, hi))
    with pytest.raises(ValueError, match="rows"):
        unet(x[lo:hi], t, rows=(lo, hi + 1))
    assert torch.equal(before, unet(x, t, down_intrablock_additional_residuals=feats).sample)


@pytest.mark.parametrize("lo,hi", [(2, 4), (1, 2)])
def test_controlnet_row_window(tiny, lo, hi):
    import mrisr
    s = setup(tiny["cfg"], 5102, rows=4)
    cnet, t = tiny["cnet"], torch.tensor(500)
    x, cc, cond = s["x"].cuda(), s["cc"].cuda(), s["cond"].cuda()
    d0, m0 = cnet(x, t, encoder_hidden_states=cc, controlnet_cond=cond, return_dict=False)
    before = [d.clone() for d in d0] + [m0.clone()]
    dw, mw = cnet(x[lo:hi], t, rows=(lo, hi), return_dict=False)
    dr, mr = tiny["o_cnet"](s["x"][lo:hi], t, encoder_hidden_states=s["cc"][lo:hi], controlnet_cond=s["cond"][lo:hi], return_dict=False)
    for k, (a, b) in enumerate(zip(list(dw) + [mw], list(dr) + [mr])):
        r = rel(a.cpu(), b)
        print(f"controlnet rows [{lo}, {hi}) of 4, residual {k}: rel {r:.3e}")
        assert r < 1e-3, (k, r)
    d1, m1 = cnet(x, t, return_dict=False)  # cached context and condition embedding
    assert all(torch.equal(a, b) for a, b in zip(before, list(d1) + [m1]))
    with pytest.raises(mrisr.MrisrError, match="inside the planned batch"):
        cnet(x[0:2], t, rows=(3, 5), return_dict=False)


# ------------------------------------------------------------------------------------------------ 3 - 7. trajectories against the oracles
def test_ddim_cfg_guidance_interval(tiny):
    """Guided steps {2, 3}, reduced steps {0, 1, 4}: 3 B + 2 * 2 B rows, two variants, two captures."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 5111)
    sp, g, phi, iv = host_scheduler("ddim"), 3.0, 0.7, (0.4, 0.8)
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_rescale=phi, guidance_interval=iv)
    assert [tuple(r) == NEUTRAL for r in rows] == [True, True, False, False, True]
    traj = osa.ddim_sample(ScheduledUNet(tiny["o_unet"], rows, "cfg", s["cc"], ctx_u=s["cu"].expand(B, -1, -1)), s["x"], None, oracle_scheduler())
    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, guidance_rescale=phi,
              guidance_interval=iv, skip_neutral=True)
    smp = check_states("ddim + cfg interval, skipping", lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim"), s["x"].cuda(), traj, N, kw)
    stats(smp, unet_rows=3 * B + 2 * 2 * B, controlnet_steps=0, feature_steps=0, variants=2, captures=2)


def test_resshift_pag_alone_with_noise(tiny):
    """Res-SRDiff, PAG alone over steps 1..3 with step noise: steps 0 and 4 forward the B conditional rows."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 5112)
    sp = host_scheduler("resshift")
    rows = mrisr.step_schedule(sp.timesteps, pag_scale=2.0, pag_interval=(0.2, 0.8))
    assert [float(r[1]) > 0 for r in rows] == [False, True, True, True, False]
    so = oracle_scheduler()
    traj = osa.res_srdiff_sample(ScheduledUNet(tiny["o_unet"], rows, "pag", s["cc"], layers=OUTER), None, s["lr"], s["cc"], None,
                                 so.timesteps, so.alphas_cumprod, s["z"][0], list(s["z"][1:]))
    x0 = mrisr.get_res_shifting_latents(s["lr"].cuda(), s["lr"].cuda(), sp.timesteps[0], sp, s["z"][0].cuda())
    assert rel(x0.cpu(), traj[0]) < 1e-5
    kw = dict(encoder_hidden_states=s["cc"].cuda(), lr_latents=s["lr"].cuda(), step_noise=s["z"][1:].cuda(), pag_scale=2.0,
              pag_applied_layers=OUTER, pag_interval=(0.2, 0.8), skip_neutral=True)
    smp = check_states("resshift + pag interval, skipping", lambda: mrisr.Sampler(tiny["unet"], sp, kind="resshift"), x0, traj, N, kw)
    stats(smp, unet_rows=2 * B + 3 * 2 * B, variants=2, captures=2)


def test_unipc_pag_and_cfg_history_survives(tiny):
    """UniPC, K = 3, both intervals end before the last two steps: the reduced steps read the ring the guided steps wrote."""
    import mrisr
    import multistep_ref as mref
    s = setup(tiny["cfg"], 5113)
    sp, g, sc = host_scheduler("unipc"), 3.0, 1.5
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, pag_scale=sc, guidance_interval=(0.0, 0.6), pag_interval=(0.0, 0.6))
    assert [tuple(r) == NEUTRAL for r in rows] == [False, False, False, True, True]
    wrapped = ScheduledUNet(tiny["o_unet"], rows, "pag+cfg", s["cc"], ctx_u=s["cu"].expand(B, -1, -1), layers=OUTER)
    traj = mref.multistep_sample("unipc", wrapped, s["x"], None, sp.timesteps, sp.alphas_cumprod, last=N)
    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, pag_scale=sc,
              pag_applied_layers=OUTER, guidance_interval=(0.0, 0.6), pag_interval=(0.0, 0.6), skip_neutral=True)
    smp = check_states("unipc + pag + cfg, skipping", lambda: mrisr.Sampler(tiny["unet"], sp, kind="unipc"), s["x"].cuda(), traj, N, kw)
    stats(smp, unet_rows=3 * 3 * B + 2 * B, variants=2, captures=2)


def test_controlnet_and_adapter_intervals(tiny):
    """control_guidance_end 0.6, adapter_conditioning_factor 0.4: the ControlNet on steps 0..2, the features on steps 0..1."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 5114)
    sp = host_scheduler("ddim")
    rows = cr.table(N, 1.0, 0.0, 0.6, 1.0, 0.4)
    traj = osa.ddim_sample(cr.ScaledAdapterUNet(tiny["o_unet"], rows), s["x"], s["cc"], oracle_scheduler(), cr.ScaledControlNet(tiny["o_cnet"], rows),
                           s["cond"], intrablock=[f.clone() for f in s["feats"]])
    kw = dict(encoder_hidden_states=s["cc"].cuda(), controlnet_cond=s["cond"].cuda(), adapter_features=[f.cuda() for f in s["feats"]],
              control_guidance_end=0.6, adapter_conditioning_factor=0.4, skip_neutral=True)
    smp = check_states("controlnet + adapter intervals, skipping", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)
    stats(smp, unet_rows=N * B, controlnet_steps=3, feature_steps=2, variants=3, captures=3)


def test_controlnet_and_adapter_guess_mode_under_cfg(tiny):
    """The same two intervals under classifier-free guidance in guess mode, guidance over steps 0..1: step 2 is a reduced step WITH the
    ControlNet (which guess mode already runs on the B conditional rows: its residuals cover the whole window), steps 3 and 4 are reduced
    steps without either network."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 5115)
    sp, g = host_scheduler("ddim"), 3.0
    cu = s["cu"].expand(B, -1, -1)
    rows8 = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_interval=(0.0, 0.4))
    rows4 = cr.table(N, 1.0, 0.0, 0.6, 1.0, 0.4)
    assert mrisr.step_variants(rows8, rows4, 2, True, 4) == [0, 0, 1 | 4, 1 | 2 | 4, 1 | 2 | 4]
    unet = cr.ScaledAdapterUNet(ScheduledUNet(PairUNet(tiny["o_unet"], cu, s["cc"]), rows8, "cfg", s["cc"], ctx_u=cu), rows4)
    traj = osa.ddim_sample(unet, s["x"], None, oracle_scheduler(), cr.ScaledControlNet(tiny["o_cnet"], rows4, guess=True, ctx_c=s["cc"]), s["cond"],
                           intrablock=[f.clone() for f in s["feats"]])
    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, guidance_interval=(0.0, 0.4),
              controlnet_cond=s["cond"].cuda(), adapter_features=[f.cuda() for f in s["feats"]], control_guidance_end=0.6,
              adapter_conditioning_factor=0.4, guess_mode=True, skip_neutral=True)
    smp = check_states("guess mode + cfg + both intervals, skipping", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)
    stats(smp, unet_rows=2 * 2 * B + 3 * B, controlnet_steps=3, feature_steps=2, variants=3, captures=3)


def test_controlnet_and_features_on_reduced_steps(tiny):
    """No conditioning table: on a reduced step the ControlNet itself forwards the row window (it is planned for all 2 B rows), and the
    features are read at the window's rows."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 5116)
    sp, g, iv = host_scheduler("ddim"), 3.0, (0.4, 0.8)
    cu = s["cu"].expand(B, -1, -1)
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_interval=iv)
    unet = ScheduledUNet(PairUNet(tiny["o_unet"], cu, s["cc"]), rows, "cfg", s["cc"], ctx_u=cu)
    traj = osa.ddim_sample(unet, s["x"], None, oracle_scheduler(), GuidedControlNet(tiny["o_cnet"], cu, s["cc"]), s["cond"],
                           intrablock=[f.clone() for f in s["feats"]])
    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, guidance_interval=iv,
              controlnet_cond=s["cond"].cuda(), adapter_features=[f.cuda() for f in s["feats"]], skip_neutral=True)
    smp = check_states("cfg interval + controlnet + features, skipping", lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim"), s["x"].cuda(), traj, N, kw)
    stats(smp, unet_rows=3 * B + 2 * 2 * B, controlnet_steps=N, feature_steps=N, variants=2, captures=2)


def test_with_tiles(tiny):
    """16 x 16 canvas, tile 8, overlap 0 (T = 4): a reduced step gathers the last part of the staging buffer and blends into the window of
    the prediction buffer; rows count tiles."""
    import mrisr
    from oracle import sampler as osa
    s = setup(tiny["cfg"], 5117)
    sp, g, phi, iv = host_scheduler("ddim"), 3.0, 0.7, (0.4, 0.8)
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_rescale=phi, guidance_interval=iv)
    wrapped = ScheduledUNet(TiledUNet(tiny["o_unet"], 16, 16, 8, 0), rows, "cfg", s["cc"], ctx_u=s["cu"].expand(B, -1, -1))
    traj = osa.ddim_sample(wrapped, s["x"], None, oracle_scheduler())

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_tiles(8, 0)
        return smp

    kw = dict(encoder_hidden_states=s["cc"].cuda(), uncond_hidden_states=s["cu"].cuda(), guidance_scale=g, guidance_rescale=phi,
              guidance_interval=iv, skip_neutral=True)
    smp = check_states("tiles + cfg interval, skipping", make, s["x"].cuda(), traj, N, kw)
    stats(smp, unet_rows=4 * (3 * B + 2 * 2 * B), variants=2, captures=2)


# ------------------------------------------------------------------------------------------------ 8 - 10. the sampler's state
def full_kw(s, **more):
    return dict(uncond_hidden_states=s["cu"].cuda(), guidance_scale=3.0, guidance_rescale=0.7, controlnet_cond=s["cond"].cuda(),
                adapter_features=[f.cuda() for f in s["feats"]], **more)


def test_graph_replay_equals_eager_launches(tiny):
    import mrisr
    s = setup(tiny["cfg"], 5121)
    sp = host_scheduler("ddim")
    kw = full_kw(s, guidance_interval=(0.4, 0.8), controlnet_conditioning_scale=0.5, control_guidance_end=0.8, adapter_conditioning_factor=0.6,
                 skip_neutral=True)
    finals = {}
    for use_graph in (True, False):
        smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
        finals[use_graph] = run(smp, s["x"].cuda(), s["cc"].cuda(), use_graph=use_graph, **kw)
        # steps: 0, 1 reduced; 2 full; 3 guided without features; 4 reduced without either network
        stats(smp, unet_rows=3 * B + 2 * 2 * B, controlnet_steps=4, feature_steps=3, variants=4, captures=4 if use_graph else 0)
    assert torch.equal(finals[True], finals[False]) and not torch.equal(finals[True], s["x"])


def test_no_neutral_row_is_the_run_without_the_option(tiny):
    import mrisr
    s = setup(tiny["cfg"], 5122)
    sp = host_scheduler("ddim")
    kw = dict(uncond_hidden_states=s["cu"].cuda(), guidance_scale=3.0, schedule=constant_rows(N, 3.0, 0.0, 0.7))
    off = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), s["x"].cuda(), s["cc"].cuda(), **kw)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    on = run(smp, s["x"].cuda(), s["cc"].cuda(), skip_neutral=True, **kw)
    assert torch.equal(on, off) and not torch.equal(on, s["x"])
    stats(smp, unet_rows=N * 2 * B, variants=1, captures=1)
    # a run without any table has nothing to skip either
    plain = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    a = run(plain, s["x"].cuda(), s["cc"].cuda(), skip_neutral=True)
    assert torch.equal(a, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), s["x"].cuda(), s["cc"].cuda()))
    stats(plain, unet_rows=N * B, variants=1, captures=1)


def test_replay_capture_counts_and_clearing_the_option(tiny):
    import mrisr
    s = setup(tiny["cfg"], 5123)
    sp = host_scheduler("ddim")
    x, cc = s["x"].cuda(), s["cc"].cuda()
    kw = full_kw(s)
    ta = mrisr.step_schedule(sp.timesteps, guidance_scale=3.0, guidance_rescale=0.7, guidance_interval=(0.4, 0.8))
    tb = ta.copy()
    tb[2:4, 0] = (2.0, 5.0)                                   # other values, the same neutral pattern
    ca = cr.constant_rows(N, 0.5, 0.8)
    cb = cr.constant_rows(N, 0.7, 0.6)
    smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    a = run(smp, x, cc, schedule=ta, conditioning=ca, skip_neutral=True, **kw)
    stats(smp, variants=2, captures=2, controlnet_steps=N, feature_steps=N)
    b = run(smp, x, cc, schedule=tb, conditioning=cb, skip_neutral=True, **kw)
    stats(smp, variants=2, captures=2)                         # nothing new
    assert not torch.equal(a, b)
    assert torch.equal(a, run(smp, x, cc, schedule=ta, conditioning=ca, skip_neutral=True, **kw))
    stats(smp, captures=2)
    cz = ca.copy()
    cz[4, 0] = 0.0                                            # step 4: reduced AND without the ControlNet - one more variant
    c = run(smp, x, cc, schedule=ta, conditioning=cz, skip_neutral=True, **kw)
    stats(smp, variants=3, captures=3, controlnet_steps=N - 1, unet_rows=3 * B + 2 * 2 * B)
    assert not torch.equal(c, a)
    # the option cleared: the full step's graph alone, the bits of a sampler that never had the option, nothing captured
    d = run(smp, x, cc, schedule=ta, conditioning=cz, **kw)
    stats(smp, variants=1, captures=3, controlnet_steps=N, unet_rows=N * 2 * B)
    fresh = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind="ddim")
    assert torch.equal(d, run(fresh, x, cc, schedule=ta, conditioning=cz, **kw))
    stats(fresh, variants=1, captures=1)
    assert rel(c, d) < TOL                                     # the same run but for rounding on the skipped steps
    assert torch.equal(c, run(smp, x, cc, schedule=ta, conditioning=cz, skip_neutral=True, **kw))
    stats(smp, variants=3, captures=3)


# ------------------------------------------------------------------------------------------------ 11. bf16
def test_reduced_ddim_step_bf16(tiny):
    """Step 0 of 5 alone on a neutral row, bf16 engine: the reduced step against the skip-off step from the same state, at
    test_gpu_guidance.py's bf16 convention (5e-2 on a single forward; g = 1: no amplification), on the state and on the prediction the
    step consumed."""
    import mrisr
    cfg = tiny["cfg"]
    s = setup(cfg, 5131)
    so = oracle_scheduler()
    rows = constant_rows(N)
    rows[1:, 0] = 2.0
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    kw = dict(uncond_hidden_states=s["cu"].cuda(), guidance_scale=2.0, schedule=rows)
    outs = {}
    for skip in (False, True):
        smp = mrisr.Sampler(net, host_scheduler("ddim"), kind="ddim")
        smp.set_range(0, 1)
        outs[skip] = run(smp, s["x"].cuda(), s["cc"].cuda(), skip_neutral=skip, **kw)
        stats(smp, unet_rows=B if skip else 2 * B, variants=1, captures=1)
    cx, ce = so.ddim_coeffs(int(so.timesteps[0]))
    e_on, e_off = ((outs[k].double() - cx * s["x"].double()) / ce for k in (True, False))
    r_x, r_e = rel(outs[True], outs[False]), rel(e_on, e_off)
    print(f"bf16 reduced DDIM step vs the skip-off step: state rel {r_x:.3e}, consumed eps rel {r_e:.3e} (bound 5e-2)")
    assert r_x < 5e-2 and r_e < 5e-2, (r_x, r_e)
    e_ref = tiny["o_unet"](s["x"], torch.tensor(int(so.timesteps[0])), encoder_hidden_states=s["cc"]).sample
    assert rel(e_on, e_ref) < 5e-2


# ------------------------------------------------------------------------------------------------ 12. refusals
def test_refusals_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    s = setup(tiny["cfg"], 5141)
    x, cu, cc = s["x"].cuda(), s["cu"].cuda(), s["cc"].cuda()
    lat = x.clone()
    sp = host_scheduler("ddim")
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    kw = dict(uncond_hidden_states=cu, guidance_scale=3.0, guidance_interval=(0.4, 0.8))
    for bad in (1, "on", None):
        with pytest.raises(ValueError, match="must be a bool"):
            smp.run(lat, cc, skip_neutral=bad, **kw)
    cached = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    cached.set_cache(2, 1)
    with pytest.raises(ValueError, match="feature cache"):
        cached.run(lat, cc, skip_neutral=True, **kw)
    # the C ABI refuses the pair in either order
    with pytest.raises(mrisr.MrisrError, match="skipping neutral steps together with a feature cache"):
        L.check(L.lib().mrisr_sampler_set_skip(cached._h, 1))
    L.check(L.lib().mrisr_sampler_set_skip(smp._h, 1))
    with pytest.raises(mrisr.MrisrError, match="skipping neutral steps together with a feature cache"):
        L.check(L.lib().mrisr_sampler_set_cache(smp._h, 2, 1))
    L.check(L.lib().mrisr_sampler_set_skip(smp._h, 0))
    with pytest.raises(mrisr.MrisrError, match="null"):
        L.check(L.lib().mrisr_sampler_run_stats(smp._h, None))
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran on the latents
    # after a skipping run, set_cache is not refused for what that run left in the library
    run(smp, x, cc, skip_neutral=True, **kw)
    smp.set_cache(2, 1)
    smp.set_cache(1, 1)
    a = run(smp, x, cc, **kw)
    assert torch.equal(a, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x, cc, **kw))
