"""GPU: low-frequency consistency in the graph sampler (ILVR; ``Sampler.run(consistency_ref=, consistency_factor=,
consistency_weight=, consistency_interval=, consistency_filter=, consistency_noise=, consistency=)``).  TINY UNet and ControlNet, f32
engine, 5 steps, latents [2, 4, 16, 16], factor 4 unless stated.

* trajectories against the CPU oracle's own step functions with the post-step hook of tests/consistency_ref.py (itself checked by
  test_consistency_cpu.py) at 1e-3 relative L2 and max-relative - the f32 tolerance of every sampler test here: every state of the five
  kinds, classifier-free guidance (K = 2), PAG with it (K = 3), ``skip_neutral`` with reduced steps, a ControlNet, tiles on a
  [1, 4, 32, 32] canvas, ``set_range`` split runs.  Each case first asserts ON THE ORACLE that its reference ends at least ten times that
  tolerance away from the run without consistency, so a device run that ignored the keywords could not pass (``oracle_case``);
* an all-zero-weight table gives the bits of the run without the keywords; graph == eager; other weights and intervals replay the stored
  graph; another factor, filter or reference buffer, and clearing, capture again;
* one bf16 step at 3 x 5e-2, test_gpu_guidance.py's convention; ``log_validation``; every refusal, before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import consistency_ref as kr
from guidance_ref import GuidedUNet
from pag_ref import PagUNet
from pag_testlib import StubVAE, maxrel, rel
from schedule_ref import ScheduledUNet
from tiles_ref import TiledUNet

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N = 5
B = 2
TOL = 1e-3
FACTOR = 4
OUTER = ("down_blocks.0", "up_blocks.3")


def oracle_nets():
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=6201, perturb_norm=True)
    cp = ou.init_controlnet_params(cfg, seed=6202, perturb_norm=True)
    return dict(cfg=cfg, p=p, cp=cp, o_unet=ou.OracleUNet(p, cfg), o_cnet=ou.OracleControlNet(cp, cfg))


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    t = oracle_nets()
    unet = mrisr.UNet2DConditionModel(t["cfg"], compute_dtype="f32")
    unet.load_state_dict(t["p"])
    cnet = mrisr.ControlNetModel(t["cfg"], compute_dtype="f32")
    cnet.load_state_dict(t["cp"])
    t.update(unet=unet, cnet=cnet)
    return t


def setup(cfg, seed, batch=B, hw=16, n=N):
    """x, LR anchor, the consistency reference, step noise and consistency noise [n, B, ...], contexts, condition image."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((batch, 4, hw, hw), generator=g)
    lr = 0.18215 * torch.randn((batch, 4, hw, hw), generator=g)
    # a reference with structure in its low band: a smooth field plus detail
    coarse = torch.randn((batch, 4, hw // 4, hw // 4), generator=g)
    ref = 0.6 * torch.nn.functional.interpolate(coarse, scale_factor=4, mode="bilinear", align_corners=False) + 0.1 * torch.randn((batch, 4, hw, hw), generator=g)
    z = torch.randn((n, batch, 4, hw, hw), generator=g)
    cz = torch.randn((n, batch, 4, hw, hw), generator=g)
    cu = torch.randn((1, 77, cfg.cross_attention_dim), generator=g)
    cc = torch.randn((batch, 77, cfg.cross_attention_dim), generator=g)
    cond = torch.randn((batch, 3, 8 * hw, 8 * hw), generator=g)
    return dict(x=x, lr=lr, ref=ref, z=z, cz=cz, cu=cu, cc=cc, cond=cond)


def host_scheduler(kind, n=N):
    import mrisr
    cls = {"ddim": mrisr.DDIMScheduler, "resshift": mrisr.DDPMScheduler, "ddpm": mrisr.DDPMScheduler, "unipc": mrisr.UniPCMultistepScheduler,
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
    return smp


def to_cuda(kw):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def oracle_case(nets, name):
    """(x0, oracle trajectory, host kind, run keywords on the CPU, n) of the named case - everything the device is compared against - after
    the effect-size guard, ON THE ORACLE ALONE: the reference ends >= 10 x the tolerance away from the same run without consistency."""
    from oracle import sampler as osa
    cfg, net, cnet = nets["cfg"], nets["o_unet"], nets["o_cnet"]
    n, so = N, oracle_scheduler()
    if name in ("ddim", "ddpm", "resshift"):
        s = setup(cfg, 6300 + len(name))
        anchored, noisy = name == "resshift", name == "resshift"
        filt, weight, iv = ("nearest", 1.0, (0.0, 1.0)) if name == "resshift" else ("bilinear", 0.5, (0.2, 1.0))
        table = kr.rows(name, so, anchored, weight, iv, noisy)
        x0 = osa.res_shift_forward(s["lr"], s["lr"], torch.tensor(int(so.timesteps[0])), so.alphas_cumprod, s["z"][0]) if anchored else s["x"]
        noise = list(s["z"][1:]) if name == "resshift" else (s["z"] if name == "ddpm" else None)
        sample = lambda hook: kr.first_order_sample(name, net, x0, s["cc"], so, hook, lr_latents=s["lr"] if anchored else None, step_noise=noise)  # noqa: E731
        hook = kr.make_hook(table, s["ref"], FACTOR, filt, s["lr"] if anchored else None, s["cz"] if noisy else None)
        kw = dict(encoder_hidden_states=s["cc"], consistency_ref=s["ref"], consistency_filter=filt, consistency_weight=weight,
                  consistency_interval=iv)
        if name == "resshift":
            kw.update(lr_latents=s["lr"], step_noise=s["z"][1:N], consistency_noise=s["cz"])
        if name == "ddpm":
            kw.update(step_noise=s["z"])
    elif name in ("unipc", "dpmsolver++"):
        s = setup(cfg, 6310 + len(name))
        anchored = name == "unipc"  # one multistep kind on z = x - LR, one on x
        sp = host_scheduler(name)
        table = kr.rows(name, so, anchored, 0.8, (0.0, 0.8))
        x0 = s["x"]
        sample = lambda hook: kr.multistep_sample(name, net, x0, s["cc"], sp.timesteps, sp.alphas_cumprod, hook=hook,  # noqa: E731
                                                  lr_latents=s["lr"] if anchored else None, last=N)
        hook = kr.make_hook(table, s["ref"], FACTOR, "bilinear", s["lr"] if anchored else None)
        kw = dict(encoder_hidden_states=s["cc"], consistency_ref=s["ref"], consistency_weight=0.8, consistency_interval=(0.0, 0.8))
        if anchored:
            kw.update(lr_latents=s["lr"])
    elif name in ("cfg", "pag+cfg", "skip"):
        s = setup(cfg, 6320 + len(name))
        g, phi, ps, cu = 3.0, 0.7, 2.0, s["cu"].expand(B, -1, -1)
        table = kr.rows("ddim", so, False, 1.0, (0.0, 0.8))
        x0 = s["x"]
        kw = dict(encoder_hidden_states=s["cc"], uncond_hidden_states=s["cu"], guidance_scale=g, guidance_rescale=phi,
                  consistency_ref=s["ref"], consistency_interval=(0.0, 0.8))
        if name == "cfg":
            wrapped = GuidedUNet(net, cu, s["cc"], g, phi)
        elif name == "pag+cfg":
            wrapped = PagUNet(net, s["cc"], ps, OUTER, ctx_u=cu, guidance_scale=g, guidance_rescale=phi)
            kw.update(pag_scale=ps, pag_applied_layers=OUTER)
        else:
            import mrisr
            rows8 = mrisr.step_schedule(host_scheduler("ddim").timesteps, guidance_scale=g, guidance_rescale=phi, guidance_interval=(0.4, 0.8))
            assert [float(r[0]) != 1.0 for r in rows8] == [False, False, True, True, False]
            wrapped = None
            kw.update(guidance_interval=(0.4, 0.8), skip_neutral=True)

        def sample(hook):
            u = wrapped if wrapped is not None else ScheduledUNet(net, rows8, "cfg", s["cc"], ctx_u=cu)  # (counts its calls: one per run)
            return kr.first_order_sample("ddim", u, x0, None, so, hook)
        hook = kr.make_hook(table, s["ref"], FACTOR)
    elif name == "controlnet":
        s = setup(cfg, 6330)
        table = kr.rows("ddim", so, False, 0.7)
        x0 = s["x"]
        sample = lambda hook: kr.first_order_sample("ddim", net, x0, s["cc"], so, hook, controlnet=cnet, control_image=s["cond"])  # noqa: E731
        hook = kr.make_hook(table, s["ref"], FACTOR, "nearest")
        kw = dict(encoder_hidden_states=s["cc"], controlnet_cond=s["cond"], consistency_ref=s["ref"], consistency_weight=0.7,
                  consistency_filter="nearest")
    else:
        assert name == "tiles"
        n = 3
        so = oracle_scheduler(n)
        s = setup(cfg, 6340, batch=1, hw=32, n=n)
        table = kr.rows("ddim", so, False, 1.0)
        x0 = s["x"]
        sample = lambda hook: kr.first_order_sample("ddim", TiledUNet(net, 32, 32, 16, 8), x0, s["cc"], so, hook)  # noqa: E731
        hook = kr.make_hook(table, s["ref"], 8)
        kw = dict(encoder_hidden_states=s["cc"], consistency_ref=s["ref"], consistency_factor=8)
    traj, plain = sample(hook), sample(None)
    d = rel(traj[n], plain[n])
    print(f"{name}: oracle with consistency vs without: rel {d:.3e} (needs >= {10 * TOL:.0e})")
    assert d >= 10 * TOL, (name, d)
    kind = name if name in ("ddim", "ddpm", "resshift", "unipc", "dpmsolver++") else "ddim"
    return x0, traj, kind, kw, n


# ------------------------------------------------------------------------------------------------ 1. trajectories
@pytest.mark.parametrize("name", ("ddim", "resshift", "ddpm", "unipc", "dpmsolver++", "cfg", "pag+cfg", "controlnet", "tiles"))
def test_trajectory(tiny, name):
    import mrisr
    x0, traj, kind, kw, n = oracle_case(tiny, name)
    sp = host_scheduler(kind, n)

    def make():
        smp = mrisr.Sampler(tiny["unet"], sp, tiny["cnet"] if name == "controlnet" else None, kind=kind)
        if name == "tiles":
            smp.set_tiles(16, 8)
        return smp
    check_states(f"consistency, {name}", make, x0.cuda(), traj, n, to_cuda(kw))


def test_trajectory_skip_neutral_keeps_the_parts_current(tiny):
    """Guided steps {2, 3}, reduced steps {0, 1, 4}: the consistency launch of a reduced step writes every part of the staging buffer, so
    the guided steps that follow read the consistent state in both halves."""
    import mrisr
    x0, traj, kind, kw, n = oracle_case(tiny, "skip")
    smp = check_states("consistency, skip_neutral", lambda: mrisr.Sampler(tiny["unet"], host_scheduler("ddim"), kind="ddim"), x0.cuda(), traj,
                       n, to_cuda(kw))
    st = smp.last_run_stats
    assert st["unet_rows"] == 3 * B + 2 * 2 * B and st["variants"] == 2, st


def test_set_range_split_run_reads_the_rows_and_slabs_of_its_steps(tiny):
    """DDIM with a noised reference, run as (0, 2) then (2, 5) on one buffer: the full run.  Rows and noise slabs are indexed by the
    absolute step: a table (or a noise stack) rolled by two steps gives another result."""
    import mrisr
    s = setup(tiny["cfg"], 6350)
    so = oracle_scheduler()
    table = kr.rows("ddim", so, False, 0.6, (0.0, 1.0), noisy=True)
    ref = kr.first_order_sample("ddim", tiny["o_unet"], s["x"], s["cc"], so, kr.make_hook(table, s["ref"], FACTOR, noise=s["cz"]))[N]
    plain = kr.first_order_sample("ddim", tiny["o_unet"], s["x"], s["cc"], so)[N]
    assert rel(ref, plain) >= 10 * TOL
    smp = mrisr.Sampler(tiny["unet"], host_scheduler("ddim"), kind="ddim")
    lat, cc, d_ref, d_cz = s["x"].cuda().clone(), s["cc"].cuda(), s["ref"].cuda(), s["cz"].cuda()
    kw = dict(consistency_ref=d_ref, consistency_weight=0.6, consistency_noise=d_cz)
    for lo, hi in ((0, 2), (2, 5)):
        smp.set_range(lo, hi)
        smp.run(lat, cc, **kw)
    torch.cuda.synchronize()
    r, m = rel(lat, ref), maxrel(lat, ref)
    print(f"consistency, set_range (0, 2) + (2, 5): rel {r:.3e} maxrel {m:.3e}")
    assert r < TOL and m < TOL
    tail = kr.first_order_sample("ddim", tiny["o_unet"], s["x"], s["cc"], so, kr.make_hook(table, s["ref"], FACTOR, noise=s["cz"]), first=2)[-1]
    smp.set_range(2, 5)
    got = run(smp, s["x"].cuda(), cc, consistency=table, consistency_ref=d_ref, consistency_noise=d_cz)
    assert rel(got, tail) < TOL and maxrel(got, tail) < TOL
    rolled = run(smp, s["x"].cuda(), cc, consistency=np.roll(table, 2, axis=0), consistency_ref=d_ref, consistency_noise=d_cz)
    assert rel(rolled, tail) > 10 * TOL
    rolled = run(smp, s["x"].cuda(), cc, consistency=table, consistency_ref=d_ref, consistency_noise=torch.roll(d_cz, 2, 0).contiguous())
    assert rel(rolled, tail) > 10 * TOL


# ------------------------------------------------------------------------------------------------ 2. the sampler's state
def test_zero_weight_table_is_the_run_without_the_keywords(tiny):
    import mrisr
    s = setup(tiny["cfg"], 6401)
    x, cc, ref = s["x"].cuda(), s["cc"].cuda(), s["ref"].cuda()
    for kind, extra in (("ddim", dict(uncond_hidden_states=s["cu"].cuda(), guidance_scale=3.0)), ("unipc", dict(lr_latents=s["lr"].cuda())),
                        ("ddim", dict())):
        sp = host_scheduler(kind)
        a = run(mrisr.Sampler(tiny["unet"], sp, kind=kind), x, cc, **extra)
        smp = mrisr.Sampler(tiny["unet"], sp, kind=kind)
        zero = np.zeros((N, 4), dtype=np.float32)
        zero[:, 1:] = (0.9, 0.1, 0.0)
        b = run(smp, x, cc, consistency_ref=ref, consistency=zero, **extra)
        c = run(smp, x, cc, consistency_ref=ref, consistency_weight=0.0, **extra)
        d = run(smp, x, cc, consistency_ref=torch.full_like(ref, float("nan")), consistency_interval=(0.5, 0.5), **extra)
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and not torch.equal(a, s["x"]), kind
        assert captures(smp) == 2  # the NaN reference is another buffer
        e = run(smp, x, cc, **extra)  # and the run without the keywords on the same sampler: cleared, the launches of before
        assert torch.equal(a, e) and captures(smp) == 3


def test_graph_replay_equals_eager_launches(tiny):
    import mrisr
    s = setup(tiny["cfg"], 6402)
    for kind, extra in (("ddim", dict(uncond_hidden_states=s["cu"].cuda(), guidance_scale=3.0, guidance_rescale=0.7)),
                        ("resshift", dict(lr_latents=s["lr"].cuda(), step_noise=s["z"][:N - 1].cuda(), consistency_noise=s["cz"].cuda(),
                                          consistency_filter="nearest"))):
        finals = {}
        for use_graph in (True, False):
            smp = mrisr.Sampler(tiny["unet"], host_scheduler(kind), kind=kind)
            finals[use_graph] = run(smp, s["x"].cuda(), s["cc"].cuda(), use_graph=use_graph, consistency_ref=s["ref"].cuda(), **extra)
            assert captures(smp) == (1 if use_graph else 0)
        assert torch.equal(finals[True], finals[False]) and not torch.equal(finals[True], s["x"]), kind


def test_what_replays_and_what_captures_again(tiny):
    import mrisr
    s = setup(tiny["cfg"], 6403)
    sp = host_scheduler("ddim")
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    x, cc, ref = s["x"].cuda(), s["cc"].cuda(), s["ref"].cuda()
    fresh = lambda **k: run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x, cc, **k)  # noqa: E731
    a = run(smp, x, cc, consistency_ref=ref)
    assert captures(smp) == 1
    b = run(smp, x, cc, consistency_ref=ref, consistency_weight=0.4)                       # another weight: the stored graph
    c = run(smp, x, cc, consistency_ref=ref, consistency_interval=(0.2, 0.6))              # another interval
    t = mrisr.consistency_schedule(sp.timesteps, sp.alphas_cumprod, "ddim", False, 2.0)
    d = run(smp, x, cc, consistency_ref=ref, consistency=t)                                # an explicit table
    assert captures(smp) == 1 and len({bytes(v.numpy().tobytes()) for v in (a, b, c, d)}) == 4
    assert torch.equal(run(smp, x, cc, consistency_ref=ref), a) and captures(smp) == 1
    assert torch.equal(b, fresh(consistency_ref=ref, consistency_weight=0.4))             # nothing stale
    ref.copy_(0.5 * s["ref"].cuda())                                                       # the SAME buffer refilled: by address, the stored graph
    e = run(smp, x, cc, consistency_ref=ref)
    assert captures(smp) == 1 and torch.equal(e, fresh(consistency_ref=0.5 * s["ref"].cuda())) and not torch.equal(e, a)
    ref.copy_(s["ref"].cuda())
    f = run(smp, x, cc, consistency_ref=ref, consistency_factor=2)                         # another factor
    assert captures(smp) == 2 and not torch.equal(f, a) and torch.equal(f, fresh(consistency_ref=ref, consistency_factor=2))
    g = run(smp, x, cc, consistency_ref=ref, consistency_factor=2, consistency_filter="nearest")  # another filter
    assert captures(smp) == 3 and not torch.equal(g, f)
    other = ref.clone()
    h = run(smp, x, cc, consistency_ref=other, consistency_factor=2, consistency_filter="nearest")  # another reference buffer
    assert captures(smp) == 4 and torch.equal(h, g)
    i = run(smp, x, cc)                                                                    # cleared
    assert captures(smp) == 5 and torch.equal(i, fresh())
    assert torch.equal(run(smp, x, cc, consistency_ref=ref), a) and captures(smp) == 6


# ------------------------------------------------------------------------------------------------ 3. bf16, log_validation, refusals
def test_consistent_ddim_step_bf16(tiny):
    """Step 1 of 5 alone (set_range(1, 2)) with the bf16 UNet against the oracle's step and hook at 3 x 5e-2 (test_gpu_guidance.py's convention
    for a bf16 step): the state, and the part of it the consistency launch does not touch at "nearest" - the detail inside each block."""
    import mrisr
    cfg = tiny["cfg"]
    s = setup(cfg, 6501)
    so = oracle_scheduler()
    table = kr.rows("ddim", so, False, 1.0)
    hook = kr.make_hook(table, s["ref"], FACTOR, "nearest")
    x_ref = kr.first_order_sample("ddim", tiny["o_unet"], s["x"], s["cc"], so, hook, first=1, last=2)[-1]
    x_pre = kr.first_order_sample("ddim", tiny["o_unet"], s["x"], s["cc"], so, None, first=1, last=2)[-1]  # the state the launch starts from
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16")
    unet.load_state_dict(tiny["p"])
    smp = mrisr.Sampler(unet, host_scheduler("ddim"), kind="ddim")
    smp.set_range(1, 2)
    lat = run(smp, s["x"].cuda(), s["cc"].cuda(), consistency_ref=s["ref"].cuda(), consistency_filter="nearest")
    pool = lambda t: torch.nn.functional.avg_pool2d(t.double(), FACTOR)  # noqa: E731
    detail = lambda t: t.double() - pool(t).repeat_interleave(FACTOR, 2).repeat_interleave(FACTOR, 3)  # noqa: E731
    r_x, r_d = rel(lat, x_ref), rel(detail(lat), detail(x_ref))
    r_p = float((pool(lat) - pool(kr.target(s["ref"], None, None, table[1]))).abs().max())
    print(f"bf16 DDIM step with consistency: state rel {r_x:.3e}, detail rel {r_d:.3e} (bound {3 * 5e-2}); pooled gap to the target {r_p:.3e}")
    assert r_x < 3 * 5e-2 and r_d < 3 * 5e-2, (r_x, r_d)
    # the low band is f32 whatever the engine: the op test's bound, with the oracle's max|x| doubled for the bf16 state the launch really saw
    assert r_p <= 1e-5 * (float(table[1][1]) * float(s["ref"].abs().max()) + 2.0 * float(x_pre.abs().max()))


def test_log_validation_keywords(tiny):
    import mrisr
    cfg, n = tiny["cfg"], 3
    gen = torch.Generator().manual_seed(6601)
    base = torch.randn((1, 1, 32, 32), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(512, 512), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    ctx = torch.randn((1, 77, cfg.cross_attention_dim), generator=gen).cuda()
    vae, acc = StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(6602)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        out = np.asarray(mrisr.log_validation(tiny["unet"], tiny["cnet"], vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx,
                                              num_inference_steps=n, **kw))
        return out, float(torch.rand(1))  # the next draw of the global stream: what the call consumed
    (plain, draw), (again, _) = panel(), panel()
    W = plain.shape[1] // 3
    assert np.array_equal(plain, again)
    assert np.array_equal(plain, panel(consistency_factor=None, consistency_weight=1.0, consistency_interval=None, consistency_filter="bilinear")[0])
    on, draw_on = panel(consistency_factor=4)
    near, _ = panel(consistency_factor=4, consistency_filter="nearest")
    late, _ = panel(consistency_factor=8, consistency_weight=0.5, consistency_interval=(0.3, 1.0))
    for p in (on, near, late):
        assert not np.array_equal(p[:, W:2 * W], plain[:, W:2 * W]) and np.array_equal(p[:, :W], plain[:, :W]) and np.array_equal(p[:, 2 * W:], plain[:, 2 * W:])
    assert not np.array_equal(on, near) and not np.array_equal(on, late) and draw_on == draw  # no consistency noise is drawn
    assert np.array_equal(plain, panel()[0])
    for kw, word in ((dict(consistency_weight=0.5), "consistency_factor"), (dict(consistency_filter="nearest"), "consistency_factor"),
                     (dict(consistency_interval=(0.0, 0.5)), "consistency_factor"), (dict(consistency_factor=3), "divide"),
                     (dict(consistency_factor=4, cache_interval=2), "cache")):
        with pytest.raises(ValueError, match=word):
            panel(**kw)


def test_refusals_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    s = setup(tiny["cfg"], 6701)
    x, cc, ref, cz = s["x"].cuda(), s["cc"].cuda(), s["ref"].cuda(), s["cz"].cuda()
    lat = x.clone()
    sp = host_scheduler("ddim")
    smp = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    good = np.tile(np.float32((1.0, 0.9, 0.0, 0.0)), (N, 1))
    noisy = np.tile(np.float32((1.0, 0.9, 0.0, 0.4)), (N, 1))
    # ---- Python, on numbers and shapes alone
    for kw, word in ((dict(consistency_factor=2), "consistency_ref"), (dict(consistency_weight=0.5), "consistency_ref"),
                     (dict(consistency_interval=(0.0, 0.5)), "consistency_ref"), (dict(consistency_filter="nearest"), "consistency_ref"),
                     (dict(consistency_noise=cz), "consistency_ref"), (dict(consistency=good), "consistency_ref"),
                     (dict(consistency_ref=ref[:1]), "shape"), (dict(consistency_ref=ref[:, :, :8]), "shape"), (dict(consistency_ref=good), "shape"),
                     (dict(consistency_ref=ref, consistency_noise=cz[:4]), "consistency_noise"),
                     (dict(consistency_ref=ref, consistency_noise=cz[:, :1]), "consistency_noise"),
                     (dict(consistency_ref=ref, consistency=good, consistency_weight=0.5), "excludes"),
                     (dict(consistency_ref=ref, consistency=good, consistency_interval=(0.0, 0.5)), "excludes"),
                     (dict(consistency_ref=ref, consistency=good[:4]), "shape"), (dict(consistency_ref=ref, consistency=noisy), "consistency_noise"),
                     (dict(consistency_ref=ref, consistency_factor=3), "divide"), (dict(consistency_ref=ref, consistency_factor=16), "2..8"),
                     (dict(consistency_ref=ref, consistency_filter="bicubic"), "consistency_filter"),
                     (dict(consistency_ref=ref, consistency_weight=-1.0), "weight"), (dict(consistency_ref=ref, consistency_weight=float("nan")), "weight"),
                     (dict(consistency_ref=ref, consistency_interval=(0.9, 0.1)), "interval")):
        with pytest.raises(ValueError, match=word):
            smp.run(lat, cc, **kw)
    cached = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    cached.set_cache(2, 1)
    with pytest.raises(ValueError, match="cache"):
        cached.run(lat, cc, consistency_ref=ref)
    big = mrisr.Sampler(tiny["unet"], sp, kind="ddim")
    with pytest.raises(ValueError, match="LDS"):
        big.run(torch.zeros((1, 4, 256, 256)).cuda(), cc[:1], consistency_ref=torch.zeros((1, 4, 256, 256)).cuda(), consistency_factor=4)
    # none of the refused calls left a table behind: the next run without the keywords is the plain run
    fresh = run(mrisr.Sampler(tiny["unet"], sp, kind="ddim"), x, cc)
    assert torch.equal(run(smp, x, cc), fresh) and captures(smp) == 1
    # ---- mrisr_sampler_set_consistency, before any device work
    t_ref, t_cz = L.as_tensor(ref), L.as_tensor(cz, shape=(N * B, 4, 16, 16))

    def set_table(s_, rows, n=None, factor=FACTOR, filt=0, ref_t=t_ref, noise_t=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        L.check(L.lib().mrisr_sampler_set_consistency(s_._h, factor, filt, rows.ctypes.data_as(C.c_void_p), len(rows) if n is None else n,
                                                      C.byref(ref_t) if ref_t is not None else None, C.byref(noise_t) if noise_t is not None else None))
    with pytest.raises(mrisr.MrisrError, match="n_steps"):
        set_table(smp, good[:4])
    for (i, c, v), word in (((3, 0, np.nan), r"row 3: weight \(w\) is not finite"), ((1, 1, np.inf), "row 1: alpha is not finite"),
                            ((0, 2, -np.inf), "row 0: beta is not finite"), ((4, 3, np.nan), "row 4: sigma is not finite")):
        t = good.copy()
        t[i, c] = v
        with pytest.raises(mrisr.MrisrError, match=word):
            set_table(smp, t, noise_t=t_cz)
    with pytest.raises(mrisr.MrisrError, match="clears"):
        set_table(smp, good, n=0)
    for kw, word in ((dict(factor=1), "2 .. 8"), (dict(factor=9), "2 .. 8"), (dict(factor=3), "must divide"), (dict(filt=2), "filter"),
                     (dict(ref_t=None), "ref must be"), (dict(ref_t=L.as_tensor(ref[:, :2].contiguous())), "latents' shape"),
                     (dict(ref_t=L.as_tensor(ref.to(torch.bfloat16))), "ref must be"), (dict(noise_t=L.as_tensor(cz[:4].contiguous(), shape=(4 * B, 4, 16, 16))), "noise must be"),
                     (dict(noise_t=L.as_tensor(cz.to(torch.bfloat16), shape=(N * B, 4, 16, 16))), "noise must be")):
        with pytest.raises(mrisr.MrisrError, match=word):
            set_table(smp, good, **kw)
    with pytest.raises(mrisr.MrisrError, match="sigma != 0 need the noise"):
        set_table(smp, noisy)
    with pytest.raises(mrisr.MrisrError, match="consistency table together with a feature cache"):
        set_table(cached, good)
    assert torch.equal(run(smp, x, cc), fresh) and captures(smp) == 1  # none of them set anything
    # ---- the run's own rules, with a table set by hand
    t_e = L.as_tensor(cc)

    def c_run(s_, latents):
        t_lat = L.as_tensor(latents)
        L.check(L.lib().mrisr_sampler_run(s_._h, C.byref(t_lat), None, None, C.byref(t_e), None, None, 0, 1, L.stream_ptr()))
    set_table(smp, good)
    other = torch.randn((B, 4, 8, 8)).cuda()
    other0 = other.clone()
    with pytest.raises(mrisr.MrisrError, match="shape of the latents"):
        c_run(smp, other)
    with pytest.raises(mrisr.MrisrError, match="feature cache"):
        L.check(L.lib().mrisr_sampler_set_cache(smp._h, 2, 1))
    torch.cuda.synchronize()
    assert torch.equal(other, other0) and torch.equal(lat, x)  # nothing ran on the latents
    L.check(L.lib().mrisr_sampler_set_consistency(smp._h, 0, 0, None, 0, None, None))  # NULL / 0 clears: the run of before
    assert torch.equal(run(smp, x, cc), fresh)
