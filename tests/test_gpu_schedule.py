"""GPU: per-step schedules of the guidance and FreeU strengths in the graph sampler (``Sampler.run(schedule=,
pag_adaptive_scale=, guidance_interval=, pag_interval=, freeu_interval=)``).  TINY UNet (+ rank-4 LoRA), f32 engine, 5 steps, latents
[2, 4, 16, 16] unless stated.

* a CONSTANT schedule is the scalar run, bit for bit: the kernels read the same numbers from the table that the scalar run hands them
  by value;
* trajectories against the CPU oracle wrapped by tests/schedule_ref.py (itself checked by test_schedule_cpu.py) at 1e-3 relative L2
  and max-relative - the f32 tolerance of every sampler test here; one bf16 step at test_gpu_guidance.py's convention, 3 x 5e-2 at g = 2;
* other values with the same flags replay the stored graph, clearing the schedule captures again; graph == eager; ``set_range`` reads
  the rows of its steps; tiles; ``log_validation``; the refusals of a run."""
import ctypes as C

import numpy as np
import pytest
import torch

import freeu_ref as fr
from pag_testlib import StubVAE, maxrel, rel
from schedule_ref import NEUTRAL, ScheduledUNet, constant_rows
from tiles_ref import TiledUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DOCS = fr.SD15_DOCS
OUTER = ("down_blocks.0", "up_blocks.3")
N = 5


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    from oracle import unet as ou
    cfg, p = fr.tiny_params()
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32", lora_rank=4, lora_alpha=4)
    unet.load_state_dict(p)
    return dict(cfg=cfg, p=p, unet=unet, o_unet=ou.OracleUNet(p, cfg))


def setup(cfg, seed, B=2, hw=16, n=N):
    """(x [B, 4, hw, hw], LR anchor, step noise [n, B, ...], uncond context [1, L, D], cond context [B, L, D]) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 4, hw, hw), generator=g)
    lr = 0.18215 * torch.randn((B, 4, hw, hw), generator=g)
    z = torch.randn((n, B, 4, hw, hw), generator=g)
    return x, lr, z, torch.randn((1, 77, cfg.cross_attention_dim), generator=g), torch.randn((B, 77, cfg.cross_attention_dim), generator=g)


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
    """One run from x0 on this sampler's own latents buffer: the latents' address is part of the graph key, and a fresh clone per run
    would leave it to the allocator whether a second run may replay the first one's graph."""
    if getattr(smp, "_test_latents", None) is None or smp._test_latents.shape != x0.shape:
        smp._test_latents = torch.empty_like(x0).contiguous()
    lat = smp._test_latents
    lat.copy_(x0)
    smp.run(lat, ctx, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


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


# ------------------------------------------------------------------------------------------------ 1. a constant schedule is the scalar run
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_constant_schedule_is_the_scalar_run_ddim_cfg(tiny, phi):
    import mrisr
    x, _, _, cu, cc = setup(tiny["cfg"], 3801)
    sp, g = host_scheduler("ddim"), 3.0
    kw = dict(uncond_hidden_states=cu.cuda(), guidance_scale=g, guidance_rescale=phi)
    a = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), cc.cuda(), **kw)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    b = run(smp, x.cuda(), cc.cuda(), schedule=constant_rows(N, g, 0.0, phi), **kw)
    assert torch.equal(a, b) and not torch.equal(a, x) and captures(smp) == 1
    c = run(smp, x.cuda(), cc.cuda(), schedule=constant_rows(N, 1.5, 0.0, phi), **kw)  # the table's values rule, not the scalar g
    assert not torch.equal(c, a) and captures(smp) == 1
    assert torch.equal(c, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), cc.cuda(), **dict(kw, guidance_scale=1.5)))


def test_constant_schedule_is_the_scalar_run_resshift_pag_alone_with_noise(tiny):
    import mrisr
    _, lr, z, _, cc = setup(tiny["cfg"], 3802)
    sp, s = host_scheduler("resshift"), 2.0
    x0 = mrisr.get_res_shifting_latents(lr.cuda(), lr.cuda(), sp.timesteps[0], sp, z[0].cuda())
    kw = dict(lr_latents=lr.cuda(), step_noise=z[:N - 1].cuda(), pag_scale=s, pag_applied_layers=OUTER)
    a = run(mrisr.Sampler(tiny["unet"], sp, kind="resshift"), x0, cc.cuda(), **kw)
    b = run(mrisr.Sampler(tiny["unet"], sp, kind="resshift"), x0, cc.cuda(), schedule=constant_rows(N, 1.0, s, 0.0), **kw)
    assert torch.equal(a, b) and not torch.equal(a, x0.cpu())


def test_constant_schedule_is_the_scalar_run_unipc_pag_and_cfg(tiny):
    import mrisr
    x, _, _, cu, cc = setup(tiny["cfg"], 3803)
    sp, g, s, phi = host_scheduler("unipc"), 3.0, 1.5, 0.7
    kw = dict(uncond_hidden_states=cu.cuda(), guidance_scale=g, guidance_rescale=phi, pag_scale=s, pag_applied_layers=OUTER)
    a = run(mrisr.Sampler(tiny["unet"], sp, kind="unipc"), x.cuda(), cc.cuda(), **kw)
    b = run(mrisr.Sampler(tiny["unet"], sp, kind="unipc"), x.cuda(), cc.cuda(), schedule=constant_rows(N, g, s, phi), **kw)
    assert torch.equal(a, b) and not torch.equal(a, x)


def test_constant_schedule_is_the_scalar_run_ddim_freeu(tiny):
    import mrisr
    x, _, _, _, cc = setup(tiny["cfg"], 3804)
    sp, unet = host_scheduler("ddim"), tiny["unet"]
    plain = run(mrisr.Sampler(unet, sp, kind="ddim"), x.cuda(), cc.cuda())
    unet.enable_freeu(*DOCS)
    try:
        a = run(mrisr.Sampler(unet, sp, kind="ddim"), x.cuda(), cc.cuda())
        smp = mrisr.Sampler(unet, sp, kind="ddim")
        b = run(smp, x.cuda(), cc.cuda(), schedule=constant_rows(N, freeu=DOCS))
        assert torch.equal(a, b) and not torch.equal(a, plain)
        # the neutral table on a UNet with FreeU on: the launches run and change nothing - the run without FreeU, bit for bit
        c = run(smp, x.cuda(), cc.cuda(), schedule=constant_rows(N))
        assert torch.equal(c, plain) and captures(smp) == 1
        # the table's pointers are gone from the handle: a plain forward takes its four values by value again
        t = torch.tensor(500)
        f1 = unet(x.cuda(), t, encoder_hidden_states=cc.cuda()).sample.cpu()
        with fr.freeu(*DOCS, tiny["cfg"]):
            ref = tiny["o_unet"](x, t, encoder_hidden_states=cc).sample
        assert rel(f1, ref) <= 1e-3
    finally:
        unet.disable_freeu()


# ------------------------------------------------------------------------------------------------ 2. against schedule_ref on the CPU oracle
def test_adaptive_pag_trajectory(tiny):
    """pag_scale 2, pag_adaptive_scale 0.003 on the timesteps 801, 601, 401, 201, 1: s = 1.403, 0.803, 0.203, then clamped to 0 twice."""
    import mrisr
    from oracle import sampler as osa
    cfg = tiny["cfg"]
    x, _, _, _, cc = setup(cfg, 3811)
    sp = host_scheduler("ddim")
    rows = mrisr.step_schedule(sp.timesteps, pag_scale=2.0, pag_adaptive_scale=0.003)
    assert rows[2, 1] > 0.0 and rows[3, 1] == 0.0 and rows[4, 1] == 0.0
    traj = osa.ddim_sample(ScheduledUNet(tiny["o_unet"], rows, "pag", cc, layers=OUTER), x, None, oracle_scheduler())
    kw = dict(encoder_hidden_states=cc.cuda(), pag_scale=2.0, pag_applied_layers=OUTER, pag_adaptive_scale=0.003)
    check_states("adaptive pag", lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), traj, N, kw)
    const = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), cc.cuda(), pag_scale=2.0, pag_applied_layers=OUTER)
    assert rel(const, traj[N]) > 1e-2  # the schedule is what is checked: the constant-scale run misses the bound by far


def test_guidance_interval_trajectory(tiny):
    """CFG with rescale over steps 1..3 of 5, the plain conditional prediction on steps 0 and 4 (through the rescale kernel at phi = 0)."""
    import mrisr
    from oracle import sampler as osa
    cfg = tiny["cfg"]
    x, _, _, cu, cc = setup(cfg, 3812)
    sp, g, phi = host_scheduler("ddim"), 3.0, 0.7
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_rescale=phi, guidance_interval=(0.2, 0.8))
    assert [tuple(r) == NEUTRAL for r in rows] == [True, False, False, False, True]
    traj = osa.ddim_sample(ScheduledUNet(tiny["o_unet"], rows, "cfg", cc, ctx_u=cu.expand(2, -1, -1)), x, None, oracle_scheduler())
    kw = dict(encoder_hidden_states=cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=g, guidance_rescale=phi, guidance_interval=(0.2, 0.8))
    check_states("guidance interval", lambda: mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), traj, N, kw)
    const = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=g,
                guidance_rescale=phi)
    assert rel(const, traj[N]) > 1e-2


def test_freeu_interval_trajectory(tiny):
    """FreeU on steps 0..2 of 5, the identity on steps 3 and 4: a plain (K = 1) run whose six FreeU launches read the table."""
    import mrisr
    from oracle import sampler as osa
    cfg, unet = tiny["cfg"], tiny["unet"]
    x, _, _, _, cc = setup(cfg, 3813)
    sp = host_scheduler("ddim")
    rows = mrisr.step_schedule(sp.timesteps, freeu=DOCS, freeu_interval=(0.0, 0.6))
    assert [tuple(r) == NEUTRAL for r in rows] == [False, False, False, True, True]
    traj = osa.ddim_sample(ScheduledUNet(tiny["o_unet"], rows, "plain", cc, freeu=True, cfg=cfg), x, None, oracle_scheduler())
    # Steps 3 and 4 hardly move a DDIM state (on the oracle the constant-FreeU trajectory ends 2.9e-4 from this one), so the states
    # cannot tell whether rows 3 and 4 were read.  The prediction that step 3 consumed can: one step from the oracle's state 3 must
    # have used the plain prediction, which FreeU would move by 8.5e-3 (both measured on the oracle)
    so = oracle_scheduler()
    t3 = int(so.timesteps[3])
    e_plain = tiny["o_unet"](traj[3], torch.tensor(t3), encoder_hidden_states=cc).sample
    with fr.freeu(*DOCS, cfg):
        e_freeu = tiny["o_unet"](traj[3], torch.tensor(t3), encoder_hidden_states=cc).sample
    assert rel(e_freeu, e_plain) > 5e-3
    unet.enable_freeu(*DOCS)
    try:
        check_states("freeu interval", lambda: mrisr.Sampler(unet, sp, kind="ddim"), x.cuda(), traj, N,
                     dict(encoder_hidden_states=cc.cuda(), freeu_interval=(0.0, 0.6)))
        smp = mrisr.Sampler(unet, sp, kind="ddim")
        smp.set_range(3, 4)
        lat = run(smp, traj[3].cuda(), cc.cuda(), freeu_interval=(0.0, 0.6))
        smp.set_range(0, 1)
        first = run(smp, x.cuda(), cc.cuda(), freeu_interval=(0.0, 0.6))
    finally:
        unet.disable_freeu()
    cx, ce = so.ddim_coeffs(t3)
    e_dev = (lat.double() - cx * traj[3].double()) / ce
    r = rel(e_dev, e_plain)
    print(f"freeu interval: the prediction step 3 consumed vs the plain one: rel {r:.3e}; FreeU would move it by {rel(e_freeu, e_plain):.3e}")
    assert r < 1e-3
    plain = run(mrisr.Sampler(unet, sp, kind="ddim"), x.cuda(), cc.cuda())  # FreeU off: the rows of steps 0..2 are what moves the run
    assert rel(plain, traj[N]) > 1e-2 and rel(first, traj[1]) < 1e-3


def test_all_three_at_once_trajectory(tiny):
    """PAG with CFG (3B rows): adaptive PAG, a guidance interval and a FreeU interval in one table."""
    import mrisr
    from oracle import sampler as osa
    cfg, unet = tiny["cfg"], tiny["unet"]
    x, _, _, cu, cc = setup(cfg, 3814)
    sp, g, phi, s, ad = host_scheduler("ddim"), 3.0, 0.7, 2.0, 0.003
    rows = mrisr.step_schedule(sp.timesteps, g, phi, s, ad, guidance_interval=(0.2, 0.8), freeu=DOCS, freeu_interval=(0.0, 0.6))
    assert len({tuple(r) for r in rows}) == N and tuple(rows[4]) == NEUTRAL  # five distinct rows, the last one neutral
    traj = osa.ddim_sample(ScheduledUNet(tiny["o_unet"], rows, "pag+cfg", cc, ctx_u=cu.expand(2, -1, -1), layers=OUTER, freeu=True, cfg=cfg),
                           x, None, oracle_scheduler())
    kw = dict(encoder_hidden_states=cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=g, guidance_rescale=phi, pag_scale=s,
              pag_applied_layers=OUTER, pag_adaptive_scale=ad, guidance_interval=(0.2, 0.8), freeu_interval=(0.0, 0.6))
    unet.enable_freeu(*DOCS)
    try:
        check_states("adaptive pag + guidance interval + freeu interval", lambda: mrisr.Sampler(unet, sp, kind="ddim"), x.cuda(), traj, N, kw)
    finally:
        unet.disable_freeu()


def test_dpmsolver_with_lr_latents_trajectory(tiny):
    """DPM-Solver++ 2M anchored on the LR latents, CFG over an interval: the multistep form of the guided step reads the table."""
    import mrisr
    import multistep_ref as mref
    cfg = tiny["cfg"]
    x, lr, _, cu, cc = setup(cfg, 3815)
    sp, g = host_scheduler("dpmsolver++"), 3.0
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_interval=(0.0, 0.6))
    wrapped = ScheduledUNet(tiny["o_unet"], rows, "cfg", cc, ctx_u=cu.expand(2, -1, -1))
    traj = mref.multistep_sample("dpmsolver++", wrapped, x, None, sp.timesteps, sp.alphas_cumprod, lr_latents=lr, last=N)
    kw = dict(encoder_hidden_states=cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=g, guidance_interval=(0.0, 0.6),
              lr_latents=lr.cuda())
    check_states("dpmsolver++ + lr + guidance interval", lambda: mrisr.Sampler(tiny["unet"], sp, kind="dpmsolver++"), x.cuda(), traj, N, kw)


def test_scheduled_ddim_step_bf16(tiny):
    """Step 1 of 5 alone (set_range(1, 2)) on a table whose row 0 is neutral and row 1 has g = 2: test_gpu_guidance.py's bf16
    convention - g eps_c - (g - 1) eps_u amplifies the single-forward bound 5e-2 by 2 g - 1 = 3."""
    import mrisr
    cfg, B, g = tiny["cfg"], 2, 2.0
    x, _, _, cu, cc = setup(cfg, 3816)
    so = oracle_scheduler()
    rows = constant_rows(N)
    rows[1, 0] = g
    t1 = int(so.timesteps[1])
    e_ref = ScheduledUNet(tiny["o_unet"], rows, "cfg", cc, ctx_u=cu.expand(B, -1, -1), first=1)(x, torch.tensor(t1)).sample
    x_ref = so.ddim_step(e_ref, t1, x)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    smp = mrisr.Sampler(net, host_scheduler("ddim"), kind="ddim")
    smp.set_range(1, 2)
    lat = run(smp, x.cuda(), cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=g, schedule=rows)
    cx, ce = so.ddim_coeffs(t1)
    e_dev = (lat.double() - cx * x.double()) / ce  # the guided prediction the step consumed
    r_x, r_e = rel(lat, x_ref), rel(e_dev, e_ref)
    print(f"bf16 scheduled DDIM step, row 1 (g = 2): state rel {r_x:.3e}, guided eps rel {r_e:.3e} (bound {3 * 5e-2})")
    assert r_x < 3 * 5e-2 and r_e < 3 * 5e-2, (r_x, r_e)


# ------------------------------------------------------------------------------------------------ 3. the sampler's state
def test_other_values_replay_the_graph_and_clearing_captures_again(tiny):
    import mrisr
    x, _, _, cu, cc = setup(tiny["cfg"], 3821)
    sp = host_scheduler("ddim")
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    kw = dict(uncond_hidden_states=cu.cuda(), guidance_scale=3.0)
    ta = np.float32([(3.0, 0, 0, 1, 1, 1, 1, 0), (2.5, 0, 0, 1, 1, 1, 1, 0), (2.0, 0, 0, 1, 1, 1, 1, 0), NEUTRAL, NEUTRAL])
    tb = ta.copy()
    tb[:, 0] = (1.0, 1.0, 4.0, 5.0, 6.0)
    a = run(smp, x.cuda(), cc.cuda(), schedule=ta, **kw)
    assert captures(smp) == 1
    b = run(smp, x.cuda(), cc.cuda(), schedule=tb, **kw)
    assert captures(smp) == 1 and not torch.equal(a, b)                     # other values, equal flags: the stored graph
    assert torch.equal(run(smp, x.cuda(), cc.cuda(), schedule=ta, **kw), a) and captures(smp) == 1
    assert torch.equal(b, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), cc.cuda(), schedule=tb, **kw))  # nothing stale
    tc = ta.copy()
    tc[1, 2] = 0.5                                                          # some phi > 0: the rescale kernel, another graph
    c = run(smp, x.cuda(), cc.cuda(), schedule=tc, **kw)
    assert captures(smp) == 2 and not torch.equal(c, a)
    d = run(smp, x.cuda(), cc.cuda(), **kw)                                 # no schedule: the launch constants rule again
    assert captures(smp) == 3
    assert torch.equal(d, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x.cuda(), cc.cuda(), **kw))
    assert torch.equal(run(smp, x.cuda(), cc.cuda(), schedule=ta, **kw), a) and captures(smp) == 4


def test_graph_replay_equals_eager_launches(tiny):
    import mrisr
    x, _, _, cu, cc = setup(tiny["cfg"], 3822)
    sp, unet = host_scheduler("ddim"), tiny["unet"]
    kw = dict(uncond_hidden_states=cu.cuda(), guidance_scale=3.0, guidance_rescale=0.7, pag_scale=2.0, pag_applied_layers=OUTER,
              pag_adaptive_scale=0.003, guidance_interval=(0.2, 0.8), freeu_interval=(0.0, 0.6))
    unet.enable_freeu(*DOCS)
    try:
        finals = {}
        for use_graph in (True, False):
            smp = mrisr.Sampler(unet, sp, kind="ddim")
            finals[use_graph] = run(smp, x.cuda(), cc.cuda(), use_graph=use_graph, **kw)
            assert captures(smp) == (1 if use_graph else 0)
        assert torch.equal(finals[True], finals[False]) and not torch.equal(finals[True], x)
    finally:
        unet.disable_freeu()


def test_set_range_reads_the_rows_of_its_steps(tiny):
    """set_range(2, 5) with five distinct rows: steps 2..4 read rows 2..4 (an absolute index, like the coefficient rows)."""
    import mrisr
    x, _, _, cu, cc = setup(tiny["cfg"], 3823)
    sp, so = host_scheduler("ddim"), oracle_scheduler()
    rows = constant_rows(N)
    rows[:, 0] = (9.0, 7.0, 3.0, 1.0, 2.0)
    wrapped = ScheduledUNet(tiny["o_unet"], rows, "cfg", cc, ctx_u=cu.expand(2, -1, -1), first=2)
    ref = x
    for t in so.timesteps.tolist()[2:]:
        ref = so.ddim_step(wrapped(ref, torch.tensor(t, dtype=torch.int64)).sample, t, ref)
    assert wrapped.calls == 3 and [r[0] for r in wrapped.used] == [3.0, 1.0, 2.0]
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    smp.set_range(2, 5)
    lat = run(smp, x.cuda(), cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=3.0, schedule=rows)
    r, m = rel(lat, ref), maxrel(lat, ref)
    print(f"set_range(2, 5) with a schedule: rel {r:.3e} maxrel {m:.3e}")
    assert r < 1e-3 and m < 1e-3
    shifted = np.roll(rows, 2, axis=0)  # rows 0..2 of this table are rows 3, 4, 0 of the other: a relative index would read these
    assert rel(run(smp, x.cuda(), cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=3.0, schedule=shifted), ref) > 1e-2


def test_with_tiles(tiny):
    """16 x 16 canvas, tile 8, overlap 0 (T = 4), 3 steps, CFG on step 1 only: the guided step stays on the canvas and reads the table."""
    import mrisr
    from oracle import sampler as osa
    cfg, n, g = tiny["cfg"], 3, 3.0
    x, _, _, cu, cc = setup(cfg, 3824)
    sp = host_scheduler("ddim", n)
    rows = mrisr.step_schedule(sp.timesteps, guidance_scale=g, guidance_rescale=0.7, guidance_interval=(0.2, 0.8))
    assert [tuple(r) == NEUTRAL for r in rows] == [True, False, True]
    wrapped = ScheduledUNet(TiledUNet(tiny["o_unet"], 16, 16, 8, 0), rows, "cfg", cc, ctx_u=cu.expand(2, -1, -1))
    traj = osa.ddim_sample(wrapped, x, None, oracle_scheduler(n))

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
        smp.set_tiles(8, 0)
        return smp

    kw = dict(encoder_hidden_states=cc.cuda(), uncond_hidden_states=cu.cuda(), guidance_scale=g, guidance_rescale=0.7, guidance_interval=(0.2, 0.8))
    check_states("tiles + guidance interval", make, x.cuda(), traj, n, kw)


# ------------------------------------------------------------------------------------------------ 4. log_validation
def test_log_validation_schedules(tiny):
    import mrisr
    cfg, n, unet = tiny["cfg"], 4, tiny["unet"]
    gen = torch.Generator().manual_seed(3831)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(128, 128), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    ctx = torch.randn((1, 77, cfg.cross_attention_dim), generator=gen).cuda()
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), generator=gen).cuda()
    vae, acc = StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(3832)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        return np.asarray(mrisr.log_validation(unet, None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx, num_inference_steps=n, **kw))

    plain = panel()
    W = plain.shape[1] // 3
    # the defaults: the panel of before, byte for byte - also with the keywords spelled out
    assert np.array_equal(plain, panel())
    assert np.array_equal(plain, panel(pag_adaptive_scale=0.0, guidance_interval=None, pag_interval=None, freeu_interval=None))
    assert np.array_equal(plain, panel(guidance_interval=(0.0, 1.0), pag_interval=(0.0, 1.0), freeu_interval=(0.0, 1.0)))
    pag = dict(pag_scale=3.0, pag_applied_layers=("down_blocks", "mid", "up_blocks"))
    const = panel(**pag)
    adaptive = panel(pag_adaptive_scale=0.004, **pag)
    assert not np.array_equal(const[:, W:2 * W], adaptive[:, W:2 * W]) and not np.array_equal(plain[:, W:2 * W], adaptive[:, W:2 * W])
    assert np.array_equal(const[:, :W], adaptive[:, :W]) and np.array_equal(const[:, 2 * W:], adaptive[:, 2 * W:])
    cfg_kw = dict(guidance_scale=4.0, guidance_rescale=0.7, uncond_embeds=ctx_u)
    const = panel(**cfg_kw)
    interval = panel(guidance_interval=(0.0, 0.5), **cfg_kw)
    assert not np.array_equal(const[:, W:2 * W], interval[:, W:2 * W]) and not np.array_equal(plain[:, W:2 * W], interval[:, W:2 * W])
    assert np.array_equal(const, panel(**cfg_kw))  # the sampler of the scheduled panel is gone: the constant panel is the one of before
    with pytest.raises(ValueError, match="enable_freeu"):
        panel(freeu_interval=(0.0, 0.5))
    fu_iv = panel(freeu=DOCS, freeu_interval=(0.0, 0.5))  # FreeU over the first half of the run, restored afterwards
    assert unet.freeu is None and not np.array_equal(plain[:, W:2 * W], fu_iv[:, W:2 * W])


# ------------------------------------------------------------------------------------------------ 5. refusals of a run
def test_run_refusals_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    x, _, _, cu, cc = setup(tiny["cfg"], 3841)
    x, cu, cc = x.cuda(), cu.cuda(), cc.cuda()
    lat = x.clone()
    sp = host_scheduler("ddim")
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    assert tiny["unet"].freeu is None
    with pytest.raises(mrisr.MrisrError, match="FreeU"):          # FreeU columns while the UNet has FreeU off
        smp.run(lat, cc, schedule=constant_rows(N, freeu=DOCS))
    with pytest.raises(mrisr.MrisrError, match="pag run"):        # s > 0 rows in a run that is not a PAG run: plain and guided
        smp.run(lat, cc, schedule=constant_rows(N, 1.0, 2.0))
    with pytest.raises(mrisr.MrisrError, match="pag run"):
        smp.run(lat, cc, uncond_hidden_states=cu, guidance_scale=3.0, schedule=constant_rows(N, 3.0, 2.0))
    with pytest.raises(mrisr.MrisrError, match="unconditional half"):  # g != 1 rows in a run without an unconditional half
        smp.run(lat, cc, schedule=constant_rows(N, 3.0))
    with pytest.raises(mrisr.MrisrError, match="unconditional half"):
        smp.run(lat, cc, pag_scale=2.0, schedule=constant_rows(N, 3.0, 2.0))
    with pytest.raises(ValueError, match="excludes"):
        smp.run(lat, cc, pag_scale=2.0, pag_adaptive_scale=0.01, schedule=constant_rows(N, 1.0, 2.0))
    with pytest.raises(ValueError, match="pag_scale"):
        smp.run(lat, cc, pag_adaptive_scale=0.01)
    with pytest.raises(ValueError, match="guidance_interval"):
        smp.run(lat, cc, guidance_interval=(0.2, 0.8))
    with pytest.raises(ValueError, match="enable_freeu"):
        smp.run(lat, cc, freeu_interval=(0.0, 0.6))
    # the feature cache with PAG stays refused, with the message of before - in Python and by the C ABI with a table set
    cached = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    cached.set_cache(2, 1)
    with pytest.raises(ValueError, match="cache"):
        cached.run(lat, cc, pag_scale=2.0, schedule=constant_rows(N, 1.0, 2.0))
    rows = constant_rows(N, 1.0, 2.0)
    L.check(L.lib().mrisr_sampler_set_schedule(cached._h, rows.ctypes.data_as(C.c_void_p), N))
    L.check(L.lib().mrisr_sampler_set_pag(cached._h, 1 << 6, 2.0))
    t_lat, t_e2 = L.as_tensor(lat), L.as_tensor(torch.cat([cc, cc]).contiguous())
    with pytest.raises(mrisr.MrisrError, match="pag run: a feature cache with interval > 1 is not supported"):
        L.check(L.lib().mrisr_sampler_run_pag(cached._h, C.byref(t_lat), None, None, C.byref(t_e2), None, None, 0, 0, 1, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran on the latents
    # a refused table does not stay behind: the next run without one is the plain run
    a = run(smp, x, cc)
    assert torch.equal(a, run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x, cc))
