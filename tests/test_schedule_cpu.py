"""CPU: per-step schedules of the guidance and FreeU strengths - the table builder ``mrisr.step_schedule``
against its stated rules (the adaptive PAG scale in closed form, the interval rule by brute force, neutral rows, dtype and shape,
the refusals), the rules of an explicit table (``mrisr.check_schedule``) and of ``Sampler.run``'s keywords, and the reference the GPU
tests compare against (tests/schedule_ref.py) against the constant-strength wrappers on a constant schedule."""
import os
import re

import numpy as np
import pytest
import torch

import freeu_ref as fr
from guidance_ref import GuidedUNet
from pag_ref import PagUNet
from schedule_ref import NEUTRAL, ScheduledUNet, constant_rows, inside

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERVALS = ((0.0, 1.0), (0.2, 0.8), (0.0, 0.5), (0.5, 0.5), (1.0, 1.0))


def trailing(n):
    import mrisr
    sp = mrisr.DDIMScheduler(timestep_spacing="trailing")
    sp.set_timesteps(n)
    return sp.timesteps.numpy().astype(np.int64)


@pytest.mark.parametrize("adaptive", [0.0, 0.002, 0.01])
def test_adaptive_column_is_the_closed_form(adaptive):
    """s_i = max(pag_scale - pag_adaptive_scale (1000 - t_i), 0) on a 20-step trailing grid; at 0.01 the clamp is reached."""
    import mrisr
    ts = trailing(20)
    assert ts[0] == 999 and len(ts) == 20 and (np.diff(ts) < 0).all()
    rows = mrisr.step_schedule(ts, pag_scale=3.0, pag_adaptive_scale=adaptive)
    want = np.maximum(3.0 - adaptive * (1000.0 - ts.astype(np.float64)), 0.0)
    # both sides round one float64 value <= 3 to float32: half an ulp of 3 is 1.2e-7
    assert np.abs(rows[:, 1].astype(np.float64) - want).max() <= 1.5e-7
    assert rows[0, 1] == np.float32(3.0 - adaptive * 1.0)
    if adaptive == 0.0:
        assert (rows[:, 1] == 3.0).all()
    if adaptive == 0.01:
        assert rows[-1, 1] == 0.0 and (rows[:, 1] == 0.0).sum() >= 2 and rows[0, 1] > 0.0  # clamped at the low-noise end
        assert (np.diff(rows[:, 1]) <= 0).all()
    assert (rows[:, 0] == 1.0).all() and (rows[:, 3:7] == 1.0).all() and (rows[:, 7] == 0.0).all()
    # another training length: the 1000 is num_train_timesteps
    rows = mrisr.step_schedule([499, 249, 0], pag_scale=2.0, pag_adaptive_scale=0.004, num_train_timesteps=500)
    assert np.abs(rows[:, 1].astype(np.float64) - np.maximum(2.0 - 0.004 * (500.0 - np.array([499.0, 249.0, 0.0])), 0.0)).max() <= 1.5e-7


@pytest.mark.parametrize("n", [1, 5, 20, 50])
@pytest.mark.parametrize("iv", INTERVALS)
def test_intervals_against_a_brute_force_loop(n, iv):
    import mrisr
    ts = trailing(n)
    lo, hi = iv
    docs = fr.SD15_DOCS
    rows = mrisr.step_schedule(ts, guidance_scale=3.0, guidance_rescale=0.7, pag_scale=2.0, guidance_interval=iv)
    rows_p = mrisr.step_schedule(ts, guidance_scale=3.0, guidance_rescale=0.7, pag_scale=2.0, pag_interval=iv)
    rows_f = mrisr.step_schedule(ts, freeu=docs, freeu_interval=iv)
    rows_all = mrisr.step_schedule(ts, guidance_scale=3.0, guidance_rescale=0.7, pag_scale=2.0, guidance_interval=iv, pag_interval=iv,
                                   freeu=docs, freeu_interval=iv)
    count = 0
    for i in range(n):
        within = i / n >= lo and (i + 1) / n <= hi
        assert within == inside(i, n, lo, hi)
        count += within
        assert rows[i, 0] == (3.0 if within else 1.0) and rows[i, 1] == 2.0 and rows[i, 2] == np.float32(0.7)
        assert rows_p[i, 1] == (2.0 if within else 0.0) and rows_p[i, 0] == 3.0 and rows_p[i, 2] == np.float32(0.7)
        assert tuple(rows_f[i, 3:7]) == (tuple(np.float32(docs)) if within else (1.0, 1.0, 1.0, 1.0))
        assert tuple(rows_f[i, :3]) == (1.0, 0.0, 0.0)
        if within:
            assert tuple(rows_all[i]) == tuple(np.float32((3.0, 2.0, 0.7) + docs + (0.0,)))
        else:  # outside every interval: the neutral row, exactly - also phi, since g == 1 and s == 0 leave nothing to rescale
            assert tuple(rows_all[i]) == NEUTRAL
    if iv == (0.0, 1.0):
        assert count == n
    if iv in ((0.5, 0.5), (1.0, 1.0)):
        assert count == 0
    if iv == (0.2, 0.8) and n == 5:
        assert count == 3


def test_neutral_rows_dtype_and_shape():
    import mrisr
    for n in (1, 7, 20):
        rows = mrisr.step_schedule(trailing(n))
        assert isinstance(rows, np.ndarray) and rows.dtype == np.float32 and rows.shape == (n, 8) and rows.flags["C_CONTIGUOUS"]
        assert all(tuple(r) == NEUTRAL for r in rows)
    assert tuple(mrisr.pipeline.NEUTRAL_ROW) == NEUTRAL
    # g == 1 and s == 0 get phi = 0 also without any interval; g != 1 keeps it
    assert mrisr.step_schedule(trailing(3), guidance_rescale=0.7)[:, 2].tolist() == [0.0, 0.0, 0.0]
    assert (mrisr.step_schedule(trailing(3), guidance_scale=2.0, guidance_rescale=0.5)[:, 2] == 0.5).all()
    # a torch tensor of timesteps is taken as well
    a = mrisr.step_schedule(torch.tensor([999, 499, 0]), pag_scale=1.0, pag_adaptive_scale=0.001)
    assert np.array_equal(a, mrisr.step_schedule([999, 499, 0], pag_scale=1.0, pag_adaptive_scale=0.001))


def test_step_schedule_refusals():
    import mrisr
    ts = trailing(5)
    for name in ("guidance_interval", "pag_interval", "freeu_interval"):
        for bad in ((0.6, 0.4), (-0.1, 0.5), (0.0, 1.1), (float("nan"), 1.0), (0.5,), "all", 0.5):
            with pytest.raises(ValueError, match=name):
                mrisr.step_schedule(ts, **{name: bad})
    for name in ("guidance_scale", "guidance_rescale", "pag_scale", "pag_adaptive_scale"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                mrisr.step_schedule(ts, **{name: bad})
    with pytest.raises(ValueError, match="pag_adaptive_scale"):
        mrisr.step_schedule(ts, pag_scale=3.0, pag_adaptive_scale=-0.001)
    with pytest.raises(ValueError, match="pag_scale"):
        mrisr.step_schedule(ts, pag_scale=-1.0)
    with pytest.raises(ValueError, match="guidance_rescale"):
        mrisr.step_schedule(ts, guidance_scale=2.0, guidance_rescale=1.5)
    with pytest.raises(ValueError, match="s2"):
        mrisr.step_schedule(ts, freeu=(0.9, float("nan"), 1.5, 1.6))
    with pytest.raises(ValueError, match="freeu"):
        mrisr.step_schedule(ts, freeu=(0.9, 0.2, 1.5))
    with pytest.raises(ValueError, match="timesteps"):
        mrisr.step_schedule([1000, 500])
    with pytest.raises(ValueError, match="timesteps"):
        mrisr.step_schedule([])


def test_explicit_table_rules():
    import mrisr
    good = constant_rows(4, 3.0, 1.0, 0.7, fr.SD15_DOCS)
    out = mrisr.check_schedule(good.tolist(), 4)
    assert out.dtype == np.float32 and out.shape == (4, 8) and np.array_equal(out, good)
    for shape in ((3, 8), (4, 7), (32,)):
        with pytest.raises(ValueError, match="shape"):
            mrisr.check_schedule(np.ones(shape, dtype=np.float32), 4)
    for col, bad, what in ((0, float("nan"), "guidance_scale"), (1, -0.5, "pag_scale"), (1, float("inf"), "pag_scale"),
                           (2, 1.5, "guidance_rescale"), (2, -0.1, "guidance_rescale"), (3, -1.0, "freeu_s1"), (4, -1.0, "freeu_s2"),
                           (5, -1.0, "freeu_b1"), (6, float("nan"), "freeu_b2"), (7, float("inf"), "padding")):
        rows = good.copy()
        rows[2, col] = bad
        with pytest.raises(ValueError, match=what):
            mrisr.check_schedule(rows, 4)


def test_run_keyword_rules_need_no_device():
    """``pipeline._build_schedule``, the function ``Sampler.run`` builds its table with, needs no sampler: ``schedule`` excludes the four
    convenience keywords; each of those needs its control to be active; none of them means no table."""
    import mrisr
    from mrisr.pipeline import _build_schedule
    unet = type("U", (), {"freeu": None})()
    table = constant_rows(5, 3.0)

    def build(schedule=None, ad=0.0, gi=None, pi=None, fi=None, g=3.0, phi=0.0, s=2.0, pag=True, uncond=True):
        return _build_schedule(5, trailing(5), 1000, unet.freeu, schedule, ad, gi, pi, fi, g, phi, s, pag, uncond)

    assert build() is None and build(gi=(0.0, 1.0), pi=(0, 1), fi=(0.0, 1.0)) is None  # none given: the call of before, no table
    assert np.array_equal(build(schedule=table), table)
    for kw, what in ((dict(ad=0.01), "pag_adaptive_scale"), (dict(gi=(0.2, 0.8)), "guidance_interval"), (dict(pi=(0.0, 0.5)), "pag_interval"),
                     (dict(fi=(0.0, 0.6)), "freeu_interval")):
        with pytest.raises(ValueError, match=what):
            build(schedule=table, **kw)
    with pytest.raises(ValueError, match="shape"):
        build(schedule=table[:4])
    with pytest.raises(ValueError, match="pag_adaptive_scale"):
        build(ad=-0.01)
    with pytest.raises(ValueError, match="pag_scale"):
        build(ad=0.01, pag=False)
    with pytest.raises(ValueError, match="pag_scale"):
        build(pi=(0.0, 0.5), pag=False)
    with pytest.raises(ValueError, match="guidance_interval"):
        build(gi=(0.2, 0.8), uncond=False)
    with pytest.raises(ValueError, match="guidance_interval"):
        build(gi=(0.2, 0.8), g=1.0)
    with pytest.raises(ValueError, match="guidance_interval"):
        build(gi=(0.8, 0.2))
    with pytest.raises(ValueError, match="enable_freeu"):
        build(fi=(0.0, 0.6))
    rows = build(ad=0.002, gi=(0.2, 0.8), phi=0.7)
    assert np.array_equal(rows, mrisr.step_schedule(trailing(5), 3.0, 0.7, 2.0, 0.002, (0.2, 0.8)))
    unet.freeu = fr.SD15_DOCS  # FreeU on: its four values fill the columns, over the whole run unless freeu_interval says otherwise
    rows = build(gi=(0.2, 0.8))
    assert all(tuple(r[3:7]) == tuple(np.float32(fr.SD15_DOCS)) for r in rows)
    rows = build(fi=(0.0, 0.6), pag=False, uncond=False, g=1.0, s=0.0)
    assert [tuple(r[3:7]) == (1.0, 1.0, 1.0, 1.0) for r in rows] == [False, False, False, True, True]
    assert all(tuple(r[:3]) == (1.0, 0.0, 0.0) for r in rows)


def test_new_symbols_are_declared():
    from mrisr import _lib
    hdr = open(os.path.join(ROOT, "include", "mrisr.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|size_t|const char\*)\s+(mrisr_[a-z0-9_]+)\(", hdr, flags=re.M))
    new = {"mrisr_sampler_set_schedule", "mrisr_op_scheduled_step", "mrisr_op_freeu_scheduled"}
    assert new <= declared and new <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.fixture(scope="module")
def tiny():
    from oracle import unet as ou
    cfg, p = fr.tiny_params()
    g = torch.Generator().manual_seed(3402)
    x = torch.randn((2, 4, 16, 16), generator=g)
    ctx_c = torch.randn((2, 77, cfg.cross_attention_dim), generator=g)
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), generator=g).expand(2, -1, -1)
    return dict(cfg=cfg, net=ou.OracleUNet(p, cfg), x=x, ctx_c=ctx_c, ctx_u=ctx_u, t=torch.tensor(500))


def test_reference_on_a_constant_schedule_is_the_constant_wrappers(tiny):
    """Every mode on a constant schedule, bit for bit: the same functions combine the same forwards.  Call i reads row first + i."""
    net, x, t, cc, cu, cfg = tiny["net"], tiny["x"], tiny["t"], tiny["ctx_c"], tiny["ctx_u"], tiny["cfg"]
    g, s, phi, layers = 3.0, 2.0, 0.7, ("mid",)
    want = GuidedUNet(net, cu, cc, g, phi)(x, t).sample
    assert torch.equal(ScheduledUNet(net, constant_rows(3, g, 0.0, phi), "cfg", cc, ctx_u=cu)(x, t).sample, want)
    want = PagUNet(net, cc, s, layers, guidance_rescale=phi)(x, t).sample
    assert torch.equal(ScheduledUNet(net, constant_rows(3, 1.0, s, phi), "pag", cc, layers=layers)(x, t).sample, want)
    want = PagUNet(net, cc, s, layers, ctx_u=cu, guidance_scale=g, guidance_rescale=phi)(x, t).sample
    assert torch.equal(ScheduledUNet(net, constant_rows(3, g, s, phi), "pag+cfg", cc, ctx_u=cu, layers=layers)(x, t).sample, want)
    with fr.freeu(*fr.SD15_DOCS, cfg):
        want = net(x, t, encoder_hidden_states=cc).sample
    plain = net(x, t, encoder_hidden_states=cc).sample
    sched = ScheduledUNet(net, constant_rows(3, freeu=fr.SD15_DOCS), "plain", cc, freeu=True, cfg=cfg)
    assert torch.equal(sched(x, t).sample, want) and not torch.equal(want, plain)
    # rows are read in call order from `first`; the neutral row is the conditional prediction
    rows = np.stack([constant_rows(1, g, 0.0, phi)[0], np.float32(NEUTRAL), constant_rows(1, 1.5, 0.0, 0.0)[0]])
    sched = ScheduledUNet(net, rows, "cfg", cc, ctx_u=cu, first=1)
    a, b = sched(x, t).sample, sched(x, t).sample
    assert sched.calls == 2 and sched.used == [[float(v) for v in rows[1]], [float(v) for v in rows[2]]]
    assert float((a - plain).norm() / plain.norm()) <= 1e-6
    assert torch.equal(b, GuidedUNet(net, cu, cc, 1.5, 0.0)(x, t).sample)
