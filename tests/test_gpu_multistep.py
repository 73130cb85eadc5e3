"""GPU: the multistep solvers (UniPC bh2, DPM-Solver++ 2M) in the graph sampler - the fused step kernel alone against the formulae in
float64, f32 trajectories against tests/multistep_ref.py driving the CPU oracle (that file is checked by test_multistep_cpu.py),
graph == eager, history zeroing, re-capture on a changed solver order, cold ranges, order 1 == DDIM, bf16, ``log_validation`` and
the errors.  f32 engine unless stated.

Tolerances: the kernel alone 1e-5 (a dozen f32 fused multiply-adds per element on O(1) coefficients; the bound the guided step
kernel meets for the same class of arithmetic); trajectories 1e-3 relative L2 and max-relative (the f32 tolerance of every sampler
test here); bf16 3 x 5e-2 (the convention of test_gpu_guidance.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import multistep_ref as mref
from guidance_ref import GuidedUNet, guided_eps

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KIND_ID = {"unipc": 3, "dpmsolver++": 4}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def maxrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def host_class(kind):
    import mrisr
    return mrisr.UniPCMultistepScheduler if kind == "unipc" else mrisr.DPMSolverMultistepScheduler


def solver_cases():
    for kind in ("unipc", "dpmsolver++"):
        for order in ((1, 2, 3) if kind == "unipc" else (1, 2)):
            yield kind, order


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def op_multistep_step(kind, x, eps, row, order, slot, hist, xc, lr=None, guided=None):
    """mrisr_op_multistep_step on copies: (new x, history, corrected state, staging buffer or None)."""
    import mrisr
    L = mrisr._lib
    x, hist = x.clone(), hist.clone()
    xc = xc.clone() if kind == "unipc" else None
    x2 = torch.full((2 * x.shape[0],) + tuple(x.shape[1:]), float("nan"), device=x.device) if guided else None
    ts = {k: L.as_tensor(v) for k, v in (("x", x), ("x2", x2), ("e", eps), ("lr", lr), ("xc", xc)) if v is not None}
    t_h = L.as_tensor(hist, shape=(hist.shape[0] * hist.shape[1],) + tuple(hist.shape[2:]))
    g, phi = guided if guided else (1.0, 0.0)
    L.check(L.lib().mrisr_op_multistep_step(KIND_ID[kind], C.byref(ts["x"]), C.byref(ts["x2"]) if guided else None, C.byref(ts["e"]),
                                            C.byref(ts["lr"]) if lr is not None else None, C.byref(t_h),
                                            C.byref(ts["xc"]) if xc is not None else None, (C.c_float * 16)(*row), order, slot, g, phi,
                                            L.stream_ptr()))
    return x, hist, xc, x2


def ref_multistep_step(kind, x, eps, row, order, slot, hist, xc, lr=None, guided=None):
    """The row layout of include/mrisr.h in float64 on the same (f32-valued) inputs."""
    B = x.shape[0]
    x, eps, hist, xc = x.double(), eps.double(), hist.double().clone(), xc.double()
    e = guided_eps(eps[:B], eps[B:], float(np.float32(guided[0])), float(np.float32(guided[1]))) if guided else eps
    z = x - (lr.double() if lr is not None else 0.0)
    h = [hist[(slot - k) % order] if k <= order else torch.zeros_like(x) for k in (1, 2, 3)]
    if kind != "unipc":
        xc = torch.zeros_like(x)
    r = [float(v) for v in row]
    m = r[0] * z + r[1] * e
    zc = r[2] * z + r[3] * e + r[4] * xc + r[5] * h[0] + r[6] * h[1] + r[7] * h[2]
    zn = r[8] * z + r[9] * e + r[10] * xc + r[11] * h[0] + r[12] * h[1] + r[13] * h[2]
    hist[slot % order] = m
    return zn + (lr.double() if lr is not None else 0.0), hist, zc


@pytest.mark.parametrize("kind,order", list(solver_cases()))
@pytest.mark.parametrize("B,Cc,h", [(1, 4, 16), (3, 4, 32), (32, 4, 32), (1, 4, 72)])
def test_multistep_step_kernel_matches_float64_formulae(kind, order, B, Cc, h):
    """Every solver x order x {plain, LR-anchored, guided with phi in {0, 0.7}}, on the rows the host class builds for a warm step
    (all history terms and the corrector live) of a 20-step trailing schedule."""
    sch = host_class(kind)(solver_order=order, timestep_spacing="trailing", final_sigmas_type="sigma_min")
    sch.set_timesteps(20)
    rows = sch.coefficient_rows()
    gen = torch.Generator().manual_seed(8000 + B * 100 + h + order)
    shape = (B, Cc, h, h)
    x = torch.randn(shape, generator=gen).cuda()
    eps2 = torch.randn((2 * B,) + shape[1:], generator=gen)
    eps2[B:] = 0.8 * eps2[B:] + 0.5 * eps2[:B] + 0.05
    eps2 = eps2.cuda()
    lr = (0.3 * torch.randn(shape, generator=gen)).cuda()
    hist = torch.randn((order,) + shape, generator=gen).cuda()
    xc = (x.cpu() + 0.05 * torch.randn(shape, generator=gen)).cuda()
    worst = 0.0
    for slot in (7, 8, 12):  # every ring position
        row = [float(np.float32(v)) for v in rows[slot]]
        assert any(row[8:14]) and (order == 1 or row[11] != 0.0)
        for anchor in (None, lr):
            for guided in (None, (3.5, 0.0), (3.5, 0.7)):
                eps = eps2 if guided else eps2[:B].contiguous()
                out, h_out, xc_out, x2 = op_multistep_step(kind, x, eps, row, order, slot, hist, xc, anchor, guided)
                ref, h_ref, xc_ref = ref_multistep_step(kind, x, eps, row, order, slot, hist, xc, anchor, guided)
                tag = (kind, order, slot, anchor is not None, guided)
                errs = [rel(out, ref), maxrel(out, ref), rel(h_out, h_ref), maxrel(h_out, h_ref)]
                if kind == "unipc":
                    errs += [rel(xc_out, xc_ref), maxrel(xc_out, xc_ref)]
                worst = max([worst] + errs)
                assert max(errs) <= 1e-5, (tag, errs)
                # only the slot of this step is written
                for k in range(order):
                    if k != slot % order:
                        assert torch.equal(h_out[k], hist[k]), tag
                if guided:
                    assert torch.equal(x2[:B], out) and torch.equal(x2[B:], out), tag
    print(f"multistep step kernel {kind} order {order} B={B} C={Cc} h={h}: worst {worst:.3e}")


# ------------------------------------------------------------------------------------------------ models
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


def scheduler(kind, n, **kw):
    sp = host_class(kind)(timestep_spacing="leading", steps_offset=1, **kw)
    sp.set_timesteps(n)
    return sp


def states(tag, make_sampler, x0, traj, n, run_kw):
    """Every state of the n-step run against ``traj``, ONE reference run of the whole schedule: set_range(0, k) stops the fused loop
    after k steps of the n-step schedule (the order schedule still counts from the schedule's end, and a step's row does not depend
    on where the run stops), so what it leaves is state k of the full run."""
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


# ------------------------------------------------------------------------------------------------ 2. trajectories
@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
@pytest.mark.parametrize("n", [8, 20])
def test_trajectory_with_lora(tiny, kind, n):
    import mrisr
    cfg, B = tiny["cfg"], 2
    _, ctx = contexts(cfg, B, 3301)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(3302))
    sp = scheduler(kind, n)
    ref_run = lambda last: mref.multistep_sample(kind, tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, last=last)  # noqa: E731
    make = lambda: mrisr.Sampler(tiny["unet"], sp, kind=kind)  # noqa: E731
    kw = dict(encoder_hidden_states=ctx.cuda())
    states(f"{kind}+lora n={n}", make, x.cuda(), ref_run(n), n, kw)


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_trajectory_with_controlnet_and_lr_anchor(tiny, kind):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 8
    _, ctx = contexts(cfg, B, 3311)
    gen = torch.Generator().manual_seed(3312)
    lr_lat = 0.18215 * torch.randn((B, 4, 16, 16), generator=gen)
    cond = torch.randn((B, 3, 128, 128), generator=gen)
    sp = scheduler(kind, n)
    x0 = mrisr.get_res_shifting_latents(lr_lat.cuda(), lr_lat.cuda(), sp.timesteps[0], sp, torch.randn(lr_lat.shape, generator=gen).cuda())
    ref_run = lambda last: mref.multistep_sample(kind, tiny["o_unet"], x0.cpu(), ctx, sp.timesteps, sp.alphas_cumprod, lr_latents=lr_lat,  # noqa: E731
                                                 controlnet=tiny["o_cnet"], control_image=cond, last=last)
    make = lambda: mrisr.Sampler(tiny["unet"], sp, tiny["cnet"], kind=kind)  # noqa: E731
    states(f"{kind}+controlnet+anchor", make, x0, ref_run(n), n, dict(encoder_hidden_states=ctx.cuda(), lr_latents=lr_lat.cuda(),
                                                                  controlnet_cond=cond.cuda()))


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_trajectory_with_adapter_features(tiny, golden_dir, kind):
    import mrisr
    from oracle import adapter as oad
    cfg, B, n = tiny["cfg"], 2, 8
    gold = np.load(os.path.join(golden_dir, "adapter_xl.npz"))
    feats = oad.adapter_forward(oad.init_adapter_params(oad.ADAPTER_TINY, seed=401), oad.ADAPTER_TINY, torch.from_numpy(gold["x"]))
    _, ctx = contexts(cfg, B, 3321)
    x = torch.randn((B, 4, 8, 8), generator=torch.Generator().manual_seed(3322))
    sp = scheduler(kind, n)
    ref_run = lambda last: mref.multistep_sample(kind, tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, intrablock=feats, last=last)  # noqa: E731
    make = lambda: mrisr.Sampler(tiny["unet"], sp, kind=kind)  # noqa: E731
    states(f"{kind}+adapter", make, x.cuda(), ref_run(n), n, dict(encoder_hidden_states=ctx.cuda(), adapter_features=[f.cuda() for f in feats]))


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_trajectory(tiny, kind, phi):
    import mrisr
    cfg, B, n, g = tiny["cfg"], 2, 8, 3.0
    ctx_u, ctx_c = contexts(cfg, B, 3331)
    gen = torch.Generator().manual_seed(3332)
    x = torch.randn((B, 4, 16, 16), generator=gen)
    lr_lat = 0.18215 * torch.randn((B, 4, 16, 16), generator=gen)
    sp = scheduler(kind, n)
    wrapped = GuidedUNet(tiny["o_unet"], ctx_u.expand(B, -1, -1), ctx_c, g, phi)
    ref_run = lambda last: mref.multistep_sample(kind, wrapped, x, None, sp.timesteps, sp.alphas_cumprod, lr_latents=lr_lat, last=last)  # noqa: E731
    make = lambda: mrisr.Sampler(tiny["unet"], sp, kind=kind)  # noqa: E731
    states(f"{kind} guided phi={phi}", make, x.cuda(), ref_run(n), n,
           dict(encoder_hidden_states=ctx_c.cuda(), uncond_hidden_states=ctx_u.cuda(), guidance_scale=g, guidance_rescale=phi,
                lr_latents=lr_lat.cuda()))


@pytest.mark.parametrize("order,final", [(3, "zero"), (3, "sigma_min"), (2, "sigma_min")])
def test_unipc_orders_final_points_and_disabled_correctors(tiny, order, final):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 8
    _, ctx = contexts(cfg, B, 3341)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(3342))
    for disable in ([], [2, 5]):
        sp = scheduler("unipc", n, solver_order=order, final_sigmas_type=final, disable_corrector=disable)
        ref = mref.multistep_sample("unipc", tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, solver_order=order,
                                    final_sigmas_type=final, disable_corrector=disable)
        states(f"unipc-{order} {final} disable={disable}", lambda: mrisr.Sampler(tiny["unet"], sp, kind="unipc"), x.cuda(), ref, n,
               dict(encoder_hidden_states=ctx.cuda()))


@pytest.mark.parametrize("n", [8, 20])
@pytest.mark.parametrize("order", [1, 2])
def test_dpmsolver_sigma_min_trajectories(tiny, n, order):
    """DPM-Solver++ ending on alphas_cumprod[0]: the last step is second order at n = 20 and drops to first order at n = 8
    (lower_order_final, n < 15) - with the "zero" final point it is first order at every n, so only these runs execute that rule in
    the library's row builder.  Every state against the reference; and the two rules differ where they should."""
    import mrisr
    cfg, B = tiny["cfg"], 2
    _, ctx = contexts(cfg, B, 3345)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(3346))
    sp = scheduler("dpmsolver++", n, solver_order=order, final_sigmas_type="sigma_min")
    assert sp.order_at(n - 1) == (2 if order == 2 and n >= 15 else 1)
    ref = mref.multistep_sample("dpmsolver++", tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, solver_order=order,
                                final_sigmas_type="sigma_min")
    states(f"2M order {order} sigma_min n={n}", lambda: mrisr.Sampler(tiny["unet"], sp, kind="dpmsolver++"), x.cuda(), ref, n,
           dict(encoder_hidden_states=ctx.cuda()))


# ------------------------------------------------------------------------------------------------ 3. the sampler's state
def plain_setup(tiny, B=2, seed=3351):
    _, ctx = contexts(tiny["cfg"], B, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, 4, 16, 16), generator=gen).cuda()
    lr = (0.18215 * torch.randn((B, 4, 16, 16), generator=gen)).cuda()
    return x, ctx.cuda(), lr


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_graph_replay_equals_eager_launches(tiny, kind):
    import mrisr
    x, ctx, lr = plain_setup(tiny)
    sp = scheduler(kind, 6)
    finals = {}
    for use_graph in (True, False):
        lat = x.clone()
        mrisr.Sampler(tiny["unet"], sp, kind=kind).run(lat, ctx, lr_latents=lr, use_graph=use_graph)
        torch.cuda.synchronize()
        finals[use_graph] = lat.cpu()
    assert torch.equal(finals[True], finals[False]) and not torch.equal(finals[True], x.cpu())


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_two_runs_on_one_sampler_agree_and_order_change_recaptures(tiny, kind):
    """The history ring and the corrected state are zeroed at the start of every run (the first step's rows carry zero coefficients
    for them, and 0 x a stale NaN is NaN): the first run is poisoned by a run on NaN latents.  Then the solver order changes between
    runs on the same sampler: each result is the fresh sampler's, bit for bit (the captured graph bakes the order in)."""
    import mrisr
    x, ctx, lr = plain_setup(tiny, seed=3361)
    sp = scheduler(kind, 6)
    one = mrisr.Sampler(tiny["unet"], sp, kind=kind)

    def run(smp, start=x):
        lat = start.clone()
        smp.run(lat, ctx, lr_latents=lr)
        torch.cuda.synchronize()
        return lat.cpu()

    a = run(one)
    assert torch.isnan(run(one, torch.full_like(x, float("nan")))).all()  # leaves NaN in the ring and in xc
    b = run(one)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    orders = (1, 2, 3, 2) if kind == "unipc" else (1, 2, 1)
    got = []
    for o in orders:
        one.set_solver(solver_order=o)
        got.append(run(one))
        fresh = mrisr.Sampler(tiny["unet"], scheduler(kind, 6, solver_order=o), kind=kind)
        assert torch.equal(got[-1], run(fresh)), o
    assert torch.equal(got[1], a) and not torch.equal(got[0], got[1])
    if kind == "unipc":
        assert not torch.equal(got[2], got[1]) and torch.equal(got[3], got[1])


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_set_range_split_starts_cold(tiny, kind):
    import mrisr
    cfg, B, n, k = tiny["cfg"], 2, 8, 3
    _, ctx = contexts(cfg, B, 3371)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(3372))
    sp = scheduler(kind, n)
    head = mref.multistep_sample(kind, tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, last=k)
    tail = mref.multistep_sample(kind, tiny["o_unet"], head[-1], ctx, sp.timesteps, sp.alphas_cumprod, first=k)
    full = mref.multistep_sample(kind, tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod)
    smp = mrisr.Sampler(tiny["unet"], sp, kind=kind)
    lat = x.cuda().clone()
    smp.set_range(0, k)
    smp.run(lat, ctx.cuda())
    smp.set_range(k, n)
    smp.run(lat, ctx.cuda())
    torch.cuda.synchronize()
    r, m = rel(lat, tail[-1]), maxrel(lat, tail[-1])
    print(f"{kind} split at {k}: vs the cold-start reference rel {r:.3e} maxrel {m:.3e}; vs the full run rel {rel(lat, full[-1]):.3e}")
    assert r < 1e-3 and m < 1e-3
    assert rel(tail[-1], full[-1]) > 1e-5  # the cold start is a different (lower-order) run: documented, not hidden


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_order_one_equals_ddim_kind(tiny, kind):
    """Order 1 (UniPC: with every corrector disabled - UniC-1 is a genuine correction) is DDIM term for term; both coefficient pairs
    are rounded from float64 expressions that agree to 1e-16, so the states agree to a few f32 ulps per step."""
    import mrisr
    x, ctx, _ = plain_setup(tiny, seed=3381)
    n = 10
    kw = dict(disable_corrector=list(range(n))) if kind == "unipc" else {}
    sp = scheduler(kind, n, solver_order=1, final_sigmas_type="sigma_min", **kw)
    sd = mrisr.DDIMScheduler(timestep_spacing="leading", steps_offset=1)
    sd.set_timesteps(n)
    a, b = x.clone(), x.clone()
    mrisr.Sampler(tiny["unet"], sp, kind=kind).run(a, ctx)
    mrisr.Sampler(tiny["unet"], sd, kind="ddim").run(b, ctx)
    torch.cuda.synchronize()
    m = maxrel(a, b)
    print(f"{kind} order 1 vs kind='ddim', {n} steps: maxrel {m:.3e}")
    assert m <= n * 8 * 2.0 ** -24  # 8 ulps per step


# ------------------------------------------------------------------------------------------------ 4. bf16
def test_unipc_bf16(tiny):
    import mrisr
    cfg, B, n = tiny["cfg"], 2, 3
    _, ctx = contexts(cfg, B, 3391)
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(3392))
    sp = scheduler("unipc", 8)
    ref = mref.multistep_sample("unipc", tiny["o_unet"], x, ctx, sp.timesteps, sp.alphas_cumprod, last=n)
    net = mrisr.UNet2DConditionModel(cfg, compute_dtype="bf16", lora_rank=4, lora_alpha=4)
    net.load_state_dict(tiny["p"])
    smp = mrisr.Sampler(net, sp, kind="unipc")
    smp.set_range(0, n)
    lat = x.cuda().clone()
    smp.run(lat, ctx.cuda())
    torch.cuda.synchronize()
    r = rel(lat, ref[-1])
    print(f"bf16 UniPC-2, {n} steps: state rel {r:.3e} (bound {3 * 5e-2})")
    assert r < 3 * 5e-2, r


# ------------------------------------------------------------------------------------------------ 5. log_validation
class _StubVAE:
    class config:
        scaling_factor = 0.18215

    def encode(self, x):
        z = torch.nn.functional.avg_pool2d(x[:, :1], 8).repeat(1, 4, 1, 1)
        return type("E", (), {"latent_dist": type("D", (), {"sample": staticmethod(lambda: z)})})

    def decode(self, z):
        return type("O", (), {"sample": torch.nn.functional.interpolate(z.mean(1, keepdim=True), scale_factor=8.0, mode="nearest")})


@pytest.mark.parametrize("kind", ["unipc", "dpmsolver++"])
def test_log_validation_with_solver_equals_the_pipeline_by_hand(tiny, kind):
    import mrisr
    cfg, n = tiny["cfg"], 4
    gen = torch.Generator().manual_seed(3401)
    base = torch.randn((1, 1, 16, 16), generator=gen)
    hr = torch.nn.functional.interpolate(base, size=(256, 256), mode="bicubic", align_corners=False).clamp(-1, 1)
    lr = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(hr, 4), scale_factor=4.0, mode="bilinear")
    _, ctx = contexts(cfg, 1, 3402)
    vae, acc = _StubVAE(), type("A", (), {"device": torch.device("cuda")})

    def panel(**kw):
        torch.manual_seed(3403)
        sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
        out = np.asarray(mrisr.log_validation(tiny["unet"], None, vae, [{"hr": hr, "lr": lr}], sched, torch.float32, acc, ctx.cuda(),
                                              num_inference_steps=n, **kw))
        return out, torch.rand(1, device="cuda").item()  # where the device RNG stream stands afterwards

    got, rng_after = panel(solver=kind)
    torch.manual_seed(3403)
    sched = mrisr.DDPMScheduler(timestep_spacing="leading", steps_offset=1)
    lr_d = lr.cuda()
    anchor = (vae.encode(lr_d.expand(-1, 3, -1, -1)).latent_dist.sample() * vae.config.scaling_factor).float()
    sched.set_timesteps(n, device="cuda")
    lat = mrisr.get_res_shifting_latents(anchor, anchor, sched.timesteps[0], sched).contiguous()
    hand_rng = torch.rand(1, device="cuda").item()  # no step noise was drawn
    mrisr.Sampler(tiny["unet"], sched, None, kind=kind).run(lat, ctx.cuda(), lr_latents=anchor)
    W = got.shape[1] // 3
    assert np.array_equal(got[:, W:2 * W], mrisr.decode_to_vis(lat, vae))
    assert rng_after == hand_rng
    plain, _ = panel()
    assert not np.array_equal(plain[:, W:2 * W], got[:, W:2 * W])
    assert np.array_equal(plain, panel(solver=None)[0])


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_are_raised_before_any_launch(tiny):
    import mrisr
    L = mrisr._lib
    x, ctx, lr = plain_setup(tiny, seed=3411)
    sp = scheduler("unipc", 4)
    with pytest.raises(ValueError):
        mrisr.Sampler(tiny["unet"], sp, kind="unipc", clip_sample_range=1.0)
    with pytest.raises(ValueError):
        mrisr.Sampler(tiny["unet"], sp, kind="dpmsolver++")  # a UniPC scheduler cannot drive the other solver
    with pytest.raises(ValueError):
        mrisr.Sampler(tiny["unet"], scheduler("dpmsolver++", 4), kind="ddim").set_solver(solver_order=2)
    smp = mrisr.Sampler(tiny["unet"], sp, kind="unipc")
    lat = x.clone()
    for kw in (dict(step_noise=torch.randn((3,) + tuple(x.shape)).cuda()), dict(lr_latents=lr[:1])):
        with pytest.raises(ValueError):
            smp.run(lat, ctx, **kw)
    with pytest.raises(ValueError):
        smp.run(torch.randn((2, 1, 3, 3)).cuda(), ctx)  # C*h*w not a multiple of 4
    for bad in (dict(solver_order=4), dict(solver_order=0), dict(final_sigmas_type="karras"), dict(disable_corrector=[-2])):
        with pytest.raises(ValueError):
            smp.set_solver(**bad)
    with pytest.raises(ValueError):
        mrisr.log_validation(tiny["unet"], None, None, [], sp, torch.float32, None, ctx, solver="euler")
    # the C ABI refuses the same things itself
    with pytest.raises(RuntimeError, match="solver_order"):
        L.check(L.lib().mrisr_sampler_set_solver(smp._h, 4, 1, 1, None, 0))
    with pytest.raises(RuntimeError, match="lower_order_final"):
        L.check(L.lib().mrisr_sampler_set_solver(smp._h, 2, 1, 0, None, 0))
    with pytest.raises(RuntimeError, match="DDPM"):
        L.check(L.lib().mrisr_sampler_set_clip(smp._h, 1.0))
    ddim = mrisr.Sampler(tiny["unet"], mrisr.DDIMScheduler(), kind="ddim")
    with pytest.raises(RuntimeError, match="multistep"):
        L.check(L.lib().mrisr_sampler_set_solver(ddim._h, 2, 1, 1, None, 0))
    nz = torch.randn((3,) + tuple(x.shape)).cuda()
    t_lat, t_e = L.as_tensor(lat), L.as_tensor(ctx.contiguous())
    t_nz = L.as_tensor(nz, shape=(nz.shape[0] * nz.shape[1],) + tuple(nz.shape[2:]))
    with pytest.raises(RuntimeError, match="step_noise"):
        L.check(L.lib().mrisr_sampler_run(smp._h, C.byref(t_lat), None, C.byref(t_nz), C.byref(t_e), None, None, 0, 1, L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(lat, x)  # nothing ran
    smp.run(lat, ctx)
    torch.cuda.synchronize()
    assert not torch.equal(lat, x) and bool(torch.isfinite(lat).all())
