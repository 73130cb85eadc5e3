"""CPU: the feature cache - the argument rules of ``Sampler.set_cache`` (``mrisr.check_cache``, no device) and the reference the GPU
tests compare against (tests/deepcache_ref.py), so that a wrong reference cannot pass unnoticed there.  TINY, B = 2, 16 x 16 latents."""
import pytest
import torch

from deepcache_ref import CachedUNet, cached_forward, num_skips

torch.set_grad_enabled(False)

B, HW = 2, 16


@pytest.fixture(scope="module")
def tiny():
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=11, perturb_norm=True)
    g = torch.Generator().manual_seed(12)
    x = torch.randn((B, 4, HW, HW), generator=g)
    ctx = torch.randn((B, 77, cfg.cross_attention_dim), generator=g)
    feats = [0.5 * torch.randn((B, c, HW >> i, HW >> i), generator=g) for i, c in enumerate(cfg.block_out_channels)]
    t = torch.tensor(601)
    full = {None: ou.unet_forward(p, cfg, x, t, ctx),
            "feats": ou.unet_forward(p, cfg, x, t, ctx, down_intrablock_additional_residuals=[f.clone() for f in feats])}
    return dict(cfg=cfg, p=p, x=x, ctx=ctx, t=t, feats=feats, full=full, n=num_skips(cfg))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_num_skips_and_depth_range(tiny):
    assert tiny["n"] == 12
    for bad in (0, 12):
        with pytest.raises(AssertionError):
            cached_forward(tiny["p"], tiny["cfg"], tiny["x"], tiny["t"], tiny["ctx"], bad)


@pytest.mark.parametrize("with_feats", [False, True])
def test_store_is_the_plain_forward_and_shallow_from_own_cache_reproduces_it(tiny, with_feats):
    """Every depth 1 .. n-1: the full (store) pass is ``oracle.unet.unet_forward`` bit for bit, and a shallow pass fed its cache at the
    same (x, t) reproduces it bit for bit.  With adapter features: depth n-1 ends on the attention-free block's last skip, which
    carries that block's feature (the in-place add); depth n-2 stops inside that block, where the feature must NOT be added."""
    cfg, p, x, t, ctx = (tiny[k] for k in ("cfg", "p", "x", "t", "ctx"))
    feats = (lambda: [f.clone() for f in tiny["feats"]]) if with_feats else (lambda: None)
    ref = tiny["full"]["feats" if with_feats else None]
    shapes = set()
    for d in range(1, tiny["n"]):
        eps, cache = cached_forward(p, cfg, x, t, ctx, d, intrablock=feats())
        assert torch.equal(eps, ref), d
        shapes.add(tuple(cache.shape))
        eps2, cache2 = cached_forward(p, cfg, x, t, ctx, d, cache=cache, intrablock=feats())
        assert torch.equal(eps2, ref), d
        assert cache2 is cache
    # depth 1 .. 11 = stages 10 .. 0: [64 | 64 | 128 (after the upsampler)] at 16, [128 | 128 | 256] at 8, [256 x 3] at 4, [256 x 2 + mid] at 2
    assert shapes == {(B, 64, 16, 16), (B, 128, 16, 16), (B, 128, 8, 8), (B, 256, 8, 8), (B, 256, 4, 4), (B, 256, 2, 2)}
    assert with_feats is False or not torch.equal(ref, tiny["full"][None])


def test_shallow_reads_the_cache_and_the_current_input(tiny):
    """A shallow pass is a function of both: another cache or another sample changes it; the deep layers it skips do not enter."""
    cfg, p, x, t, ctx = (tiny[k] for k in ("cfg", "p", "x", "t", "ctx"))
    eps, cache = cached_forward(p, cfg, x, t, ctx, 2)
    other, _ = cached_forward(p, cfg, x, t, ctx, 2, cache=cache + 0.1)
    assert rel(other, eps) > 1e-3
    moved, _ = cached_forward(p, cfg, x + 0.1, torch.tensor(580), ctx, 2, cache=cache)
    assert rel(moved, eps) > 1e-3
    q = dict(p)
    for k in q:
        if k.startswith("mid_block.") or k.startswith("down_blocks.3.") or k.startswith("up_blocks.0."):
            q[k] = torch.full_like(q[k], float("nan"))
    same, _ = cached_forward(q, cfg, x, t, ctx, 2, cache=cache)
    assert torch.equal(same, eps)


def ddim_run(unet, x, ctx, n=6):
    from oracle import sampler as osa
    from oracle import schedulers as osch
    so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
    so.set_timesteps(n)
    return osa.ddim_sample(unet, x, ctx, so)


def test_cached_unet_schedule_and_trajectories(tiny):
    from oracle import unet as ou
    cfg, p, x, ctx = (tiny[k] for k in ("cfg", "p", "x", "ctx"))
    plain = ddim_run(ou.OracleUNet(p, cfg), x, ctx)
    # interval 1: no cache at all
    one = CachedUNet(p, cfg, 1, 1)
    traj = ddim_run(one, x, ctx)
    assert all(torch.equal(a, b) for a, b in zip(traj, plain)) and one.kinds == ["full"] * 6
    # interval 3 / depth 1: the condition that lets the GPU test prove the cache is used - a cached run is >= 10x the 1e-3 sampler
    # tolerance away from the uncached one
    net = CachedUNet(p, cfg, 3, 1)
    traj = ddim_run(net, x, ctx)
    assert net.kinds == ["full", "shallow", "shallow", "full", "shallow", "shallow"]
    assert torch.equal(traj[1], plain[1]) and not torch.equal(traj[2], plain[2])  # the first step is full
    r = rel(traj[-1], plain[-1])
    print(f"TINY 6-step DDIM, interval 3 / depth 1 vs uncached: rel L2 {r:.3e}")
    assert 1e-2 <= r <= 0.2, r
    # a second run after reset() is the first one; without it the schedule would go on from step 6
    net.reset()
    again = ddim_run(net, x, ctx)
    assert all(torch.equal(a, b) for a, b in zip(again, traj))
    # interval 2: [F S F S F S]; deeper caches deviate less here
    net2 = CachedUNet(p, cfg, 2, 5)
    r2 = rel(ddim_run(net2, x, ctx)[-1], plain[-1])
    assert net2.kinds == ["full", "shallow"] * 3 and 0 < r2 < r, (r2, r)
    # two calls per step (guidance): slot k of every step keeps a cache of its own
    two = CachedUNet(p, cfg, 2, 1, calls_per_step=2)
    for k in range(4):
        two(x + k, torch.tensor(601), encoder_hidden_states=ctx)
    assert two.kinds == ["full", "full", "shallow", "shallow"]
    e0, c0 = cached_forward(p, cfg, x, torch.tensor(601), ctx, 1)
    assert torch.equal(two.caches[0], c0) and not torch.equal(two.caches[1], c0)


def test_check_cache_rules():
    import numpy as np

    import mrisr
    chk = mrisr.check_cache
    assert chk(1, 1, 12, False) == (1, 1)
    assert chk(3, 11, 12, False) == (3, 11)
    assert chk(np.int64(2), np.int32(5), 12) == (2, 5) and all(type(v) is int for v in chk(np.int64(2), np.int32(5), 12))
    assert chk(1, 1, 12, True) == (1, 1)  # interval 1 is no cache: a ControlNet is fine
    for interval, depth, n, cn in ((0, 1, 12, False), (-2, 1, 12, False), (2.0, 1, 12, False), (True, 1, 12, False), ("2", 1, 12, False),
                                   (2, 0, 12, False), (2, 12, 12, False), (2, 1.0, 12, False), (2, False, 12, False), (2, None, 12, False),
                                   (1, 12, 12, False), (2, 3, 3, False), (2, 1, 12, True), (5, 11, 12, True)):
        with pytest.raises(ValueError):
            chk(interval, depth, n, cn)
    # trailing-keyword compatibility of log_validation: the cache options are keywords with defaults that change nothing
    import inspect
    sig = inspect.signature(mrisr.log_validation).parameters
    assert sig["cache_interval"].default == 1 and sig["cache_depth"].default == 1
    sig = inspect.signature(mrisr.Sampler.set_cache).parameters
    assert sig["interval"].default == 1 and sig["depth"].default == 1
