"""GPU: when the graph sampler captures its step again.  The step graph is reused exactly when the plan of the new run (StepPlan,
csrc/step_plan.h: everything the captured launches take by value or by pointer) equals the plan it was captured from.  One long-lived
sampler goes through configurations that differ from the one before in ONE baked-in thing; after each change the capture counter must
rise by exactly the expected amount, the result must be bit-equal to the same call on a fresh sampler, and an immediate repeat must
capture nothing and give the same bits.

TINY UNet, f32 engine, latents [2, 4, 16, 16], 3 steps.  The expected counts are conditions read off the capture rule, not measurements:
1 for a changed plan, 2 when the new configuration has a feature cache (a full + store graph and a shallow one)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N_STEPS = 3


@pytest.fixture(scope="module")
def tiny():
    import mrisr
    from oracle import unet as ou
    cfg = ou.TINY
    unet = mrisr.UNet2DConditionModel(cfg, compute_dtype="f32")
    unet.load_state_dict(ou.init_unet_params(cfg, seed=2601, perturb_norm=True))
    g = torch.Generator().manual_seed(2602)
    return dict(cfg=cfg, unet=unet, x0=torch.randn((2, 4, 16, 16), generator=g).cuda(),
                ctx=torch.randn((2, 77, cfg.cross_attention_dim), generator=g).cuda(),
                uncond=torch.randn((1, 77, cfg.cross_attention_dim), generator=g).cuda())


def host_scheduler(kind):
    import mrisr
    cls = {"ddim": mrisr.DDIMScheduler, "ddpm": mrisr.DDPMScheduler, "unipc": mrisr.UniPCMultistepScheduler}[kind]
    sp = cls(timestep_spacing="leading", steps_offset=1)
    sp.set_timesteps(N_STEPS)
    return sp


def captures(smp):
    import mrisr
    return int(mrisr._lib.lib().mrisr_sampler_num_captures(smp._h))


def configure(smp, rng=(0, N_STEPS), tiles=None, cache=(1, 1), clip=None, solver=None):
    """The whole setter state of one configuration, in an order every transition allows (tiles and a cache exclude each other).  A setter
    called with the values already set drops no graph."""
    import mrisr
    smp.set_range(*rng)
    if tiles is None:
        smp.set_tiles(None)
    smp.set_cache(*cache)
    if tiles is not None:
        smp.set_tiles(*tiles)
    if clip is not None:
        mrisr._lib.check(mrisr._lib.lib().mrisr_sampler_set_clip(smp._h, C.c_float(clip)))
    if solver is not None:
        smp.set_solver(*solver)


def walk(tiny, kind, steps):
    """steps: (name, setter state, latents buffer, start values, run arguments, expected captures)."""
    import mrisr
    smp = mrisr.Sampler(tiny["unet"], host_scheduler(kind), kind=kind)
    for name, state, lat, x0, run_kw, expect in steps:
        fresh = mrisr.Sampler(tiny["unet"], host_scheduler(kind), kind=kind)  # first: whatever it re-plans on the shared UNet is done
        configure(fresh, **state)
        ref = x0.clone()
        fresh.run(ref, **run_kw)
        torch.cuda.synchronize()
        assert captures(fresh) == (2 if state.get("cache", (1, 1))[0] > 1 else 1), name
        configure(smp, **state)
        before = captures(smp)
        for what in ("after the change", "repeated"):
            lat.copy_(x0)  # the same buffer: the latents' address is part of the plan
            smp.run(lat, **run_kw)
            torch.cuda.synchronize()
            print(f"{kind} / {name} / {what}: captures +{captures(smp) - before} (expected +{expect})")
            assert captures(smp) - before == expect, (kind, name, what)
            assert torch.equal(lat, ref), (kind, name, what)
        del fresh


def test_ddim_sampler_captures_again_exactly_when_a_baked_in_value_changes(tiny):
    x0, ctx, uncond = tiny["x0"], tiny["ctx"], tiny["uncond"]
    lat, other, lat1 = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0[:1])
    plain = dict(encoder_hidden_states=ctx)
    guided = lambda g, phi: dict(encoder_hidden_states=ctx, uncond_hidden_states=uncond, guidance_scale=g, guidance_rescale=phi)
    base = dict()
    walk(tiny, "ddim", [
        ("first run", base, lat, x0, plain, 1),                                  # no graph yet
        ("guidance on", base, lat, x0, guided(3.0, 0.0), 1),                     # K 1 -> 2: the [2B] forward, the staging buffer, g
        ("guidance scale", base, lat, x0, guided(5.0, 0.0), 1),                  # g is a kernel argument
        ("guidance rescale", base, lat, x0, guided(5.0, 0.7), 1),                # phi is a kernel argument (and selects the kernel)
        ("guidance off", base, lat, x0, plain, 1),                               # K 2 -> 1
        ("other latents tensor", base, other, x0, plain, 1),                     # another data pointer
        ("batch 2 -> 1", base, lat1, x0[:1], dict(encoder_hidden_states=ctx[:1]), 1),  # B (and the UNet's workspace generation)
        ("batch 1 -> 2", base, lat, x0, plain, 1),
        ("set_range(1, 3)", dict(rng=(1, 3)), lat, x0, plain, 1),                # the first step: row 0 of the time-embedding table
        ("set_range(0, 3)", base, lat, x0, plain, 1),
        ("set_tiles(8, 0)", dict(tiles=(8, 0)), lat, x0, plain, 1),              # four 8 x 8 tiles: gather, an [8]-row forward, blend
        ("tiles off", base, lat, x0, plain, 1),
        ("set_cache(2, 1)", dict(cache=(2, 1)), lat, x0, plain, 2),              # the full + store graph and the shallow graph
        ("set_cache(1, 1)", base, lat, x0, plain, 1),
    ])


def test_ddpm_sampler_captures_again_when_the_clip_range_changes(tiny):
    x0, ctx = tiny["x0"], tiny["ctx"]
    lat = torch.empty_like(x0)
    plain = dict(encoder_hidden_states=ctx)
    walk(tiny, "ddpm", [
        ("first run", dict(clip=0.0), lat, x0, plain, 1),
        ("clip_sample_range 0 -> 1", dict(clip=1.0), lat, x0, plain, 1),         # a kernel argument; mrisr_sampler_set_clip drops the graph
        ("clip_sample_range 1 -> 0.5", dict(clip=0.5), lat, x0, plain, 1),
    ])


def test_unipc_sampler_captures_again_when_the_solver_options_change(tiny):
    x0, ctx = tiny["x0"], tiny["ctx"]
    lat = torch.empty_like(x0)
    plain = dict(encoder_hidden_states=ctx)
    walk(tiny, "unipc", [
        ("first run", dict(solver=(2, "zero", ())), lat, x0, plain, 1),
        ("solver order 2 -> 3", dict(solver=(3, "zero", ())), lat, x0, plain, 1),          # a kernel argument and the ring's slabs
        ("disable_corrector (1,)", dict(solver=(3, "zero", (1,))), lat, x0, plain, 1),     # policy: lives in the uploaded rows; set_solver
                                                                                            # promises the capture all the same
    ])
