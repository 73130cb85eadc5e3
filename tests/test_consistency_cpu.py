"""CPU: low-frequency consistency on numbers alone - ``mrisr.consistency_schedule`` against the rows
tests/consistency_ref.py reads off the oracle scheduler for every kind, every refusal of the three check functions, the properties of
the reference filter itself (the nearest filter is a projection; at w = 1 the pooled state is the pooled target), the hooked reference
loops against the oracle's own loops, and the refusals of the library that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import consistency_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ddim", "resshift", "ddpm", "unipc", "dpmsolver++")
torch.set_grad_enabled(False)


def oracle_scheduler(n, spacing="leading", offset=1):
    from oracle import schedulers as osch
    so = osch.OracleScheduler(timestep_spacing=spacing, steps_offset=offset)
    so.set_timesteps(n)
    return so


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("anchored", (False, True))
@pytest.mark.parametrize("noisy", (False, True))
def test_consistency_schedule_against_the_oracle_rows(kind, anchored, noisy):
    import mrisr
    for n, offset in ((5, 1), (10, 0), (1, 1)):
        so = oracle_scheduler(n, offset=offset)
        for final in (("zero", "sigma_min") if kind in ("unipc", "dpmsolver++") else ("zero",)):
            want = kr.rows(kind, so, anchored, 0.75, (0.0, 1.0), noisy, final)
            got = mrisr.consistency_schedule(so.timesteps, so.alphas_cumprod, kind, anchored, 0.75, noisy=noisy, final_sigmas_type=final)
            assert got.dtype == np.float32 and got.shape == (n, 4) and got.flags["C_CONTIGUOUS"]
            assert np.array_equal(got[:, 0], want[:, 0])
            assert np.allclose(got, want, rtol=0, atol=2.0 ** -23), (kind, n, final, np.abs(got - want).max())
            if not anchored:
                assert (got[:, 2] == 0).all()
            if not noisy:
                assert (got[:, 3] == 0).all()
    # the last row: the point the step rule of the kind lands on
    so = oracle_scheduler(5)
    a0 = float(so.alphas_cumprod[0])
    for final, want in (("zero", 1.0 if kind in ("ddpm", "unipc", "dpmsolver++") else a0 ** 0.5), ("sigma_min", 1.0 if kind == "ddpm" else a0 ** 0.5)):
        row = mrisr.consistency_schedule(so.timesteps, so.alphas_cumprod, kind, True, final_sigmas_type=final)[-1]
        assert row[1] == np.float32(want) and row[2] == np.float32(1.0 - want)


def test_consistency_schedule_intervals():
    import mrisr
    so = oracle_scheduler(5)
    for iv, want in (((0.0, 1.0), [2, 2, 2, 2, 2]), ((0.2, 0.8), [0, 2, 2, 2, 0]), ((0.0, 0.5), [2, 2, 0, 0, 0]), ((0.5, 1.0), [0, 0, 0, 2, 2]),
                     ((0.3, 0.3), [0, 0, 0, 0, 0])):
        got = mrisr.consistency_schedule(so.timesteps, so.alphas_cumprod, "ddim", False, 2.0, iv)
        assert got[:, 0].tolist() == [float(v) for v in want], iv
        assert np.array_equal(got, kr.rows("ddim", so, False, 2.0, iv)) or np.allclose(got, kr.rows("ddim", so, False, 2.0, iv), rtol=0, atol=2.0 ** -23)
    # the weight column follows the `inside` rule of step_schedule: the same steps as a guidance interval
    sched = mrisr.step_schedule(so.timesteps, guidance_scale=3.0, guidance_interval=(0.2, 0.8))
    got = mrisr.consistency_schedule(so.timesteps, so.alphas_cumprod, "ddim", False, 1.0, (0.2, 0.8))
    assert ((sched[:, 0] != 1) == (got[:, 0] != 0)).all()


def test_consistency_schedule_refusals():
    import mrisr
    so = oracle_scheduler(5)
    ts, ac = so.timesteps, so.alphas_cumprod
    for kw, word in ((dict(kind="euler"), "kind"), (dict(weight=-0.5), "weight"), (dict(weight=float("nan")), "weight"),
                     (dict(weight=float("inf")), "weight"), (dict(interval=(0.8, 0.2)), "interval"), (dict(interval=(0.0, 1.5)), "interval"),
                     (dict(interval=(float("nan"), 1.0)), "interval"), (dict(interval=0.5), "interval"), (dict(final_sigmas_type="one"), "final_sigmas_type")):
        args = dict(kind="ddim", anchored=False)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            mrisr.consistency_schedule(ts, ac, **args)
    with pytest.raises(ValueError, match="timesteps"):
        mrisr.consistency_schedule([], ac, "ddim", False)
    with pytest.raises(ValueError, match="timesteps"):
        mrisr.consistency_schedule([5000, 10], ac, "ddim", False)
    with pytest.raises(ValueError, match="alphas_cumprod"):
        mrisr.consistency_schedule(ts, [0.9, float("nan")], "ddim", False)


def test_check_consistency():
    import mrisr
    assert mrisr.check_consistency(4, "bilinear", 16, 16) == (4, 0)
    assert mrisr.check_consistency(np.int64(2), "nearest", 128, 128) == (2, 1)   # 48 KB: the largest accepted need at N = 2
    assert mrisr.check_consistency(8, "nearest", 256, 256) == (8, 1)
    assert mrisr.check_consistency(3, "bilinear", 6, 6) == (3, 0)
    for args, word in (((1, "bilinear", 16, 16), "consistency_factor"), ((9, "bilinear", 72, 72), "consistency_factor"),
                       ((4.0, "bilinear", 16, 16), "consistency_factor"), ((True, "bilinear", 16, 16), "consistency_factor"),
                       ((4, "bicubic", 16, 16), "consistency_filter"), ((4, 0, 16, 16), "consistency_filter"),
                       ((4, "bilinear", 18, 16), "divide"), ((4, "bilinear", 16, 18), "divide"), ((3, "bilinear", 16, 16), "divide"),
                       ((2, "bilinear", 256, 256), "LDS"), ((4, "bilinear", 256, 256), "LDS"), ((4, "bilinear", 0, 16), "h of the latents"),
                       ((4, "bilinear", 16, 4.0), "w of the latents")):
        with pytest.raises(ValueError, match=word):
            mrisr.check_consistency(*args)
    with pytest.raises(ValueError, match="feature cache"):
        mrisr.check_consistency(4, "bilinear", 16, 16, cache_interval=2)


def test_check_consistency_table():
    import mrisr
    t = np.tile(np.asarray((1.0, 0.5, 0.5, 0.0)), (5, 1))
    out = mrisr.check_consistency_table(t, 5)
    assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, t.astype(np.float32))
    assert np.array_equal(mrisr.check_consistency_table(t.tolist(), 5), out)
    for bad, word in ((t[:4], "shape"), (t[:, :3], "shape"), (t.ravel(), "shape"), ("abc", "numbers")):
        with pytest.raises(ValueError, match=word):
            mrisr.check_consistency_table(bad, 5)
    for c, name in enumerate(("weight", "alpha", "beta", "sigma")):
        for v in (np.nan, np.inf, 1e39):
            b = t.copy()
            b[2, c] = v
            with pytest.raises(ValueError, match=rf"column {c} \({name}\)"):
                mrisr.check_consistency_table(b, 5)
    neg = t.copy()
    neg[:, 0] = -1.0  # an explicit table may push away from the reference: only finiteness is asked
    assert np.array_equal(mrisr.check_consistency_table(neg, 5), neg.astype(np.float32))


def test_signatures_and_symbols():
    import inspect

    import mrisr
    from mrisr import _lib
    # the new keywords follow skip_neutral (the tails of both signatures are pinned by the earlier features' tests)
    run = list(inspect.signature(mrisr.Sampler.run).parameters.items())
    at = [k for k, _ in run].index("skip_neutral") + 1
    assert [(k, p.default) for k, p in run[at:at + 7]] == [
        ("consistency_ref", None), ("consistency_factor", 4), ("consistency_weight", 1.0), ("consistency_interval", None),
        ("consistency_filter", "bilinear"), ("consistency_noise", None), ("consistency", None)]
    lv = list(inspect.signature(mrisr.log_validation).parameters.items())
    at = [k for k, _ in lv].index("skip_neutral") + 1
    assert [(k, p.default) for k, p in lv[at:at + 4]] == [("consistency_factor", None), ("consistency_weight", 1.0), ("consistency_interval", None),
                                                          ("consistency_filter", "bilinear")]
    hdr = open(os.path.join(ROOT, "include", "mrisr.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|size_t|const char\*)\s+(mrisr_[a-z0-9_]+)\(", hdr, flags=re.M))
    new = {"mrisr_sampler_set_consistency", "mrisr_op_consistency"}
    assert new <= declared and new <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ the reference filter
@pytest.mark.parametrize("h,w,N", ((2, 2, 2), (6, 6, 3), (12, 20, 4), (16, 16, 8), (10, 15, 5), (14, 7, 7), (12, 18, 6)))
def test_nearest_phi_is_a_projection(h, w, N):
    g = torch.Generator().manual_seed(100 * h + w)
    d = torch.randn((2, 3, h, w), generator=g, dtype=torch.float64)
    p = kr.phi(d, N, "nearest")
    assert torch.equal(p, F.avg_pool2d(d, N).repeat_interleave(N, dim=2).repeat_interleave(N, dim=3))  # torch's nearest IS the block copy
    assert float((kr.phi(p, N, "nearest") - p).abs().max()) <= 1e-15                                   # idempotent
    assert float((F.avg_pool2d(p, N) - F.avg_pool2d(d, N)).abs().max()) <= 1e-15
    b = kr.phi(d, N, "bilinear")
    assert b.shape == d.shape and not torch.equal(b, p)
    # bilinear phi is linear and keeps a constant
    assert float((kr.phi(torch.full_like(d, 0.7), N) - 0.7).abs().max()) <= 1e-15
    assert float((kr.phi(2.0 * d + p, N) - (2.0 * b + kr.phi(p, N))).abs().max()) <= 1e-13


def test_bilinear_phi_is_the_stated_coordinate_rule():
    """source coordinate (i + 0.5) / N - 0.5, negative clamped to 0, upper neighbour clamped to the last cell - written out in 1-D."""
    N, nc = 4, 3
    D = torch.tensor([1.0, -2.0, 5.0], dtype=torch.float64)
    want = []
    for i in range(N * nc):
        s = max((i + 0.5) / N - 0.5, 0.0)
        i0 = int(np.floor(s))
        i1 = min(i0 + 1, nc - 1)
        lam = s - i0
        want.append((1 - lam) * float(D[i0]) + lam * float(D[i1]))
    d = D.repeat_interleave(N).reshape(1, 1, 1, -1).expand(1, 1, N, -1).contiguous()  # block means are D, one coarse row
    got = kr.phi(d, N)[0, 0, 0]
    assert float((got - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-15


def test_apply_properties():
    g = torch.Generator().manual_seed(7)
    x, ref, lr, z = (torch.randn((2, 4, 12, 20), generator=g) for _ in range(4))
    row = np.float32((1.0, 0.8, 0.2, 0.6))
    for N in (2, 4):
        out = kr.apply(x, ref, lr, z, row, N, "nearest")
        y = kr.target(ref, lr, z, row)
        assert out.dtype == torch.float64
        assert float((F.avg_pool2d(out, N) - F.avg_pool2d(y, N)).abs().max()) <= 1e-14        # data consistency at w = 1
        assert float((out - F.avg_pool2d(out, N).repeat_interleave(N, 2).repeat_interleave(N, 3)
                      - (x.double() - kr.phi(x, N, "nearest"))).abs().max()) <= 1e-14           # the detail of x is untouched
    assert torch.equal(kr.target(ref, None, None, row), float(row[1]) * ref.double())
    assert torch.equal(kr.target(ref, lr, z, np.float32((1.0, 0.8, 0.2, 0.0))), kr.target(ref, lr, None, row))
    nan = torch.full_like(x, float("nan"))
    assert torch.equal(kr.apply(x, nan, nan, nan, np.float32((0.0, 1.0, 1.0, 1.0)), 4), x.double())  # w == 0: x itself
    half = kr.apply(x, ref, lr, z, np.float32((0.5, 0.8, 0.2, 0.6)), 4)
    full = kr.apply(x, ref, lr, z, row, 4)
    assert float((half - 0.5 * (x.double() + full)).abs().max()) <= 1e-14


# ------------------------------------------------------------------------------------------------ the hooked loops
class _Net:
    """A small deterministic stand-in for the UNet: the loops, not the network, are under test."""

    class _Out:
        def __init__(self, sample):
            self.sample = sample

    def __call__(self, x, t, encoder_hidden_states=None, **kw):
        return self._Out(torch.tanh(0.7 * x + 0.001 * float(t)) + 0.1 * x.roll(1, -1))


def test_hooked_loops_without_a_hook_are_the_oracle_loops():
    from oracle import sampler as osa
    g = torch.Generator().manual_seed(11)
    x, lr = torch.randn((2, 4, 8, 8), generator=g), 0.2 * torch.randn((2, 4, 8, 8), generator=g)
    z = torch.randn((5, 2, 4, 8, 8), generator=g)
    so, net = oracle_scheduler(5), _Net()
    for a, b in zip(kr.first_order_sample("ddim", net, x, None, so), osa.ddim_sample(net, x, None, so)):
        assert torch.equal(a, b)
    for a, b in zip(kr.first_order_sample("ddpm", net, x, None, so, step_noise=z), osa.ddpm_sample(net, x, None, so, z)):
        assert torch.equal(a, b)
    want = osa.res_srdiff_sample(net, None, lr, None, None, so.timesteps, so.alphas_cumprod, z[0], list(z[1:]))
    got = kr.first_order_sample("resshift", net, want[0], None, so, lr_latents=lr, step_noise=list(z[1:]))
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == 6
    # a split run of a first-order kind, also across the stochastic steps' noise counter
    tail = kr.first_order_sample("resshift", net, want[2], None, so, lr_latents=lr, step_noise=list(z[1:]), first=2)
    assert all(torch.equal(a, b) for a, b in zip(tail, want[2:]))


@pytest.mark.parametrize("kind", ("unipc", "dpmsolver++"))
@pytest.mark.parametrize("anchored", (False, True))
def test_hooked_multistep_loop(kind, anchored):
    import multistep_ref as mref
    g = torch.Generator().manual_seed(13)
    x, lr = torch.randn((2, 4, 8, 8), generator=g), 0.2 * torch.randn((2, 4, 8, 8), generator=g)
    so, net = oracle_scheduler(5), _Net()
    lr_arg = lr if anchored else None
    plain = mref.multistep_sample(kind, net, x, None, so.timesteps, so.alphas_cumprod, lr_latents=lr_arg)
    seen = []

    def identity(i, s):
        seen.append(i)
        return s
    same = kr.multistep_sample(kind, net, x, None, so.timesteps, so.alphas_cumprod, hook=identity, lr_latents=lr_arg)
    assert seen == [0, 1, 2, 3, 4] and all(torch.equal(a, b) for a, b in zip(same, plain))
    # a hook that replaces the state: the next step starts from it, the history keeps what the step computed
    table = kr.rows(kind, so, anchored, 1.0, (0.0, 0.6))
    hook = kr.make_hook(table, lr, 4, "nearest", lr=lr_arg)
    traj = kr.multistep_sample(kind, net, x, None, so.timesteps, so.alphas_cumprod, hook=hook, lr_latents=lr_arg)
    assert torch.equal(traj[0], plain[0]) and not torch.equal(traj[1], plain[1])
    y1 = kr.target(lr, lr_arg, None, table[0])
    assert float((F.avg_pool2d(traj[1].double(), 4) - F.avg_pool2d(y1, 4)).abs().max()) <= 1e-6
    seen.clear()
    kr.multistep_sample(kind, net, x, None, so.timesteps, so.alphas_cumprod, hook=identity, lr_latents=lr_arg, first=2, last=4)
    assert seen == [2, 3]


# ------------------------------------------------------------------------------------------------ the library, no device
def test_library_refusals_that_need_no_device():
    import mrisr
    L = mrisr._lib
    lib = L.lib()
    rows = np.tile(np.float32((1.0, 1.0, 0.0, 0.0)), (5, 1))
    assert lib.mrisr_sampler_set_consistency(None, 4, 0, rows.ctypes.data_as(C.c_void_p), 5, None, None) != 0
    assert "null sampler" in lib.mrisr_last_error().decode()
    assert lib.mrisr_sampler_set_consistency(None, 0, 0, None, 0, None, None) != 0
    # mrisr_op_consistency refuses on numbers alone, before anything is launched: the pointers below are never dereferenced
    p = 4096
    good = dict(x=p, xK=p, K=2, ref=p, lr=None, noise=None, table=p, step=p, B=1, C=1, h=16, w=16, factor=4, filter=0)
    for change, word in ((dict(x=None), "null operand"), (dict(ref=None), "null operand"), (dict(table=None), "null operand"),
                         (dict(step=None), "null operand"), (dict(K=0), "K must lie in 1 .. 3"), (dict(K=4), "K must lie in 1 .. 3"),
                         (dict(xK=None), "staging buffer"), (dict(factor=1), "2 .. 8"), (dict(factor=9, h=18, w=18), "2 .. 8"),
                         (dict(filter=2), "filter"), (dict(filter=-1), "filter"), (dict(h=18), "must divide"), (dict(w=6), "must divide"),
                         (dict(h=256, w=256, factor=2), "LDS"), (dict(h=256, w=256, factor=4), "LDS"), (dict(B=0), "batch"),
                         (dict(x=p + 2), "4-byte aligned"), (dict(noise=p + 1), "4-byte aligned")):
        a = dict(good)
        a.update(change)
        rc = lib.mrisr_op_consistency(a["x"], a["xK"], a["K"], a["ref"], a["lr"], a["noise"], a["table"], a["step"], a["B"], a["C"], a["h"],
                                      a["w"], a["factor"], a["filter"], None)
        assert rc != 0 and word in lib.mrisr_last_error().decode(), (change, lib.mrisr_last_error().decode())
