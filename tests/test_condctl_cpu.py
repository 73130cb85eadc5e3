"""CPU: the conditioning strength of the graph sampler - the table builder ``mrisr.conditioning_schedule`` against its
two rules by brute force, neutral rows, dtype and shape, the rules of an explicit table (``mrisr.check_conditioning``), the guess-mode
weights, the keyword positions of ``Sampler.run`` / ``log_validation``, and the reference the GPU tests compare against
(tests/condctl_ref.py) against the unwrapped oracle: all scales 1 is the plain run and c = 0 is the run without a ControlNet, bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import condctl_ref as cr
from guidance_ref import GuidedControlNet, GuidedUNet

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (0.0, 0.1, 0.2, 0.25, 1.0 / 3.0, 0.5, 0.6, 0.8, 0.95, 1.0)


def test_conditioning_schedule_by_brute_force():
    import mrisr
    for n in range(1, 21):
        for start in GRID:
            for end in GRID:
                if end < start:
                    continue
                rows = mrisr.conditioning_schedule(n, 0.5, start, end)
                want = [np.float32(0.5) if (i / n >= start and (i + 1) / n <= end) else np.float32(0.0) for i in range(n)]
                assert rows[:, 0].tolist() == want and (rows[:, 1] == 1.0).all() and (rows[:, 2:] == 0.0).all(), (n, start, end)
                assert np.array_equal(rows, cr.table(n, 0.5, start, end))
        for factor in GRID:
            rows = mrisr.conditioning_schedule(n, adapter_conditioning_scale=0.6, adapter_conditioning_factor=factor)
            want = [np.float32(0.6) if i < int(n * factor) else np.float32(0.0) for i in range(n)]
            assert rows[:, 1].tolist() == want and (rows[:, 0] == 1.0).all() and (rows[:, 2:] == 0.0).all(), (n, factor)
            assert np.array_equal(rows, cr.table(n, a=0.6, factor=factor))


def test_neutral_rows_dtype_shape_contiguity():
    import mrisr
    rows = mrisr.conditioning_schedule(7)
    assert rows.dtype == np.float32 and rows.shape == (7, 4) and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows, np.tile(np.float32([1, 1, 0, 0]), (7, 1))) and np.array_equal(rows, cr.constant_rows(7))
    rows = mrisr.conditioning_schedule(5, 0.5, 0.2, 0.8, 0.6, 0.6)
    assert rows[:, 0].tolist() == [0.0, 0.5, 0.5, 0.5, 0.0] and rows[:, 1].tolist() == [np.float32(0.6)] * 3 + [0.0, 0.0]
    assert mrisr.conditioning_schedule(3, -1.5)[:, 0].tolist() == [-1.5] * 3  # a negative scale is a number like any other


def test_conditioning_schedule_refusals():
    import mrisr
    for kw, word in ((dict(n_steps=0), "n_steps"), (dict(n_steps=True), "n_steps"), (dict(n_steps=2.0), "n_steps"),
                     (dict(controlnet_conditioning_scale=float("nan")), "controlnet_conditioning_scale"),
                     (dict(controlnet_conditioning_scale=float("inf")), "controlnet_conditioning_scale"),
                     (dict(controlnet_conditioning_scale=1e39), "float32"),
                     (dict(adapter_conditioning_scale="x"), "adapter_conditioning_scale"),
                     (dict(control_guidance_start=0.8, control_guidance_end=0.2), "start"),
                     (dict(control_guidance_start=-0.1), "start"), (dict(control_guidance_end=1.5), "start"),
                     (dict(adapter_conditioning_factor=1.5), "adapter_conditioning_factor"),
                     (dict(adapter_conditioning_factor=-0.5), "adapter_conditioning_factor")):
        with pytest.raises(ValueError, match=word):
            mrisr.conditioning_schedule(**dict(dict(n_steps=5), **kw))


def test_check_conditioning():
    import mrisr
    good = cr.table(5, 0.5, 0.2, 0.8, 0.6, 0.6)
    out = mrisr.check_conditioning(good.astype(np.float64).tolist(), 5)
    assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, good)
    for bad, word in ((good[:4], "shape"), (good[:, :3], "shape"), (good.reshape(-1), "shape"), ("rows", "numbers")):
        with pytest.raises(ValueError, match=word):
            mrisr.check_conditioning(bad, 5)
    for col, val, word in ((0, np.nan, "column 0"), (1, np.inf, "column 1"), (2, 1.0, "column 2"), (3, -0.5, "column 3"), (2, np.nan, "column 2")):
        t = good.copy()
        t[3, col] = val
        with pytest.raises(ValueError, match=word):
            mrisr.check_conditioning(t, 5)


def test_guess_mode_weights():
    import mrisr
    w = mrisr.guess_mode_weights(12)
    assert w.dtype == np.float32 and w.shape == (13,)
    assert np.array_equal(w, np.logspace(-1, 0, 13).astype(np.float32)) and w[0] == np.float32(0.1) and w[-1] == 1.0
    assert np.abs(w.astype(np.float64) - cr.guess_weights(12).double().numpy()).max() <= 6e-8  # half an ulp of 1 in f32
    assert mrisr.guess_mode_weights(0).tolist() == [1.0]
    with pytest.raises(ValueError):
        mrisr.guess_mode_weights(-1)


def test_signature_tails():
    import mrisr
    seven = ["controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end", "adapter_conditioning_scale",
             "adapter_conditioning_factor", "guess_mode"]
    names = list(inspect.signature(mrisr.Sampler.run).parameters)
    assert names[-11:] == seven + ["conditioning", "use_graph", "guidance_scale", "guidance_rescale", "uncond_hidden_states"]
    sig = inspect.signature(mrisr.Sampler.run).parameters
    assert [sig[k].default for k in seven] == [1.0, 0.0, 1.0, 1.0, 1.0, False] and sig["conditioning"].default is None
    names = list(inspect.signature(mrisr.log_validation).parameters)
    assert names[-9:] == seven + ["guidance_scale", "guidance_rescale", "uncond_embeds"]
    assert names[:10] == ["unet", "controlnet", "vae", "val_dataloader", "noise_scheduler", "weight_dtype", "accelerator", "fixed_embeds",
                          "num_inference_steps", "adapter"]
    sig = inspect.signature(mrisr.log_validation).parameters
    assert [sig[k].default for k in seven] == [1.0, 0.0, 1.0, 1.0, 1.0, False]


def test_new_symbols_are_declared():
    from mrisr import _lib
    hdr = open(os.path.join(ROOT, "include", "mrisr.h")).read()
    declared = set(re.findall(r"^(?:int|void|int64_t|size_t|const char\*)\s+(mrisr_[a-z0-9_]+)\(", hdr, flags=re.M))
    new = {"mrisr_sampler_set_conditioning", "mrisr_op_cond_add"}
    assert new <= declared and new <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.fixture(scope="module")
def tiny():
    from oracle import schedulers as osch
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=4101, perturb_norm=True)
    cp = ou.init_controlnet_params(cfg, seed=4102, perturb_norm=True)
    g = torch.Generator().manual_seed(4103)
    x = torch.randn((2, 4, 8, 8), generator=g)
    ctx = torch.randn((2, 77, cfg.cross_attention_dim), generator=g)
    ctx_u = torch.randn((1, 77, cfg.cross_attention_dim), generator=g).expand(2, -1, -1)
    cond = torch.randn((2, 3, 64, 64), generator=g)
    feats = [torch.randn((2, c, 8 >> i, 8 >> i), generator=g) for i, c in enumerate(cfg.block_out_channels)]

    def sched(n=3):
        so = osch.OracleScheduler(timestep_spacing="leading", steps_offset=1)
        so.set_timesteps(n)
        return so
    return dict(cfg=cfg, net=ou.OracleUNet(p, cfg), cnet=ou.OracleControlNet(cp, cfg), x=x, ctx=ctx, ctx_u=ctx_u, cond=cond, feats=feats,
                sched=sched)


def test_wrappers_at_scale_one_are_the_unwrapped_run(tiny):
    from oracle import sampler as osa
    net, cnet, x, ctx, cond, feats, n = tiny["net"], tiny["cnet"], tiny["x"], tiny["ctx"], tiny["cond"], tiny["feats"], 3
    want = osa.ddim_sample(net, x, ctx, tiny["sched"](), cnet, cond, intrablock=feats)
    wc, wu = cr.ScaledControlNet(cnet, cr.constant_rows(n)), cr.ScaledAdapterUNet(net, cr.constant_rows(n))
    got = osa.ddim_sample(wu, x, ctx, tiny["sched"](), wc, cond, intrablock=feats)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and wc.calls == n and wu.calls == n
    assert wc.used == [1.0] * n and wu.used == [1.0] * n
    # rows are read in call order from `first`
    rows = cr.constant_rows(5)
    rows[:, 0] = (9, 8, 0.5, 0.25, 7)
    rows[:, 1] = (9, 8, 0.75, 0.5, 7)
    wc, wu = cr.ScaledControlNet(cnet, rows, first=2), cr.ScaledAdapterUNet(net, rows, first=2)
    for _ in range(2):
        d, m = wc(x, torch.tensor(500), encoder_hidden_states=ctx, controlnet_cond=cond)
        wu(x, torch.tensor(500), encoder_hidden_states=ctx, down_intrablock_additional_residuals=feats)
    assert wc.used == [0.5, 0.25] and wu.used == [0.75, 0.5]
    d1, m1 = cnet(x, torch.tensor(500), encoder_hidden_states=ctx, controlnet_cond=cond, return_dict=False)
    assert torch.equal(m, m1 * 0.25) and all(torch.equal(a, b * 0.25) for a, b in zip(d, d1))


def test_scale_zero_is_the_run_without_a_controlnet(tiny):
    from oracle import sampler as osa
    net, cnet, x, ctx, cond, n = tiny["net"], tiny["cnet"], tiny["x"], tiny["ctx"], tiny["cond"], 3
    want = osa.ddim_sample(net, x, ctx, tiny["sched"]())
    got = osa.ddim_sample(net, x, ctx, tiny["sched"](), cr.ScaledControlNet(cnet, cr.constant_rows(n, c=0.0)), cond)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    full = osa.ddim_sample(net, x, ctx, tiny["sched"](), cnet, cond)
    assert not torch.equal(full[-1], want[-1])
    # a = 0 likewise: the run without features
    feats = tiny["feats"]
    got = osa.ddim_sample(cr.ScaledAdapterUNet(net, cr.constant_rows(n, a=0.0)), x, ctx, tiny["sched"](), intrablock=feats)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_guess_mode_reference(tiny):
    """Unguided: the weights alone.  Under guidance: the pair form - zeros for the unconditional half, the conditional context's weighted
    residuals for the other - which GuidedUNet consumes; against the same by hand."""
    net, cnet, x, ctx, cu, cond = tiny["net"], tiny["cnet"], tiny["x"], tiny["ctx"], tiny["ctx_u"], tiny["cond"]
    t = torch.tensor(500)
    d1, m1 = cnet(x, t, encoder_hidden_states=ctx, controlnet_cond=cond, return_dict=False)
    w = np.logspace(-1, 0, len(d1) + 1)
    d, m = cr.ScaledControlNet(cnet, cr.constant_rows(1, c=0.5), guess=True)(x, t, encoder_hidden_states=ctx, controlnet_cond=cond)
    for k in range(len(d1)):
        assert float((d[k] - d1[k] * (w[k] * 0.5)).abs().max()) <= 1e-6 * float(d1[k].abs().max())
    assert torch.equal(m, m1 * 0.5)
    (du, dc), (mu, mc) = cr.ScaledControlNet(cnet, cr.constant_rows(1), guess=True, ctx_c=ctx)(x, t, encoder_hidden_states=None, controlnet_cond=cond)
    assert all(float(z.abs().max()) == 0.0 for z in du) and float(mu.abs().max()) == 0.0 and torch.equal(mc, m1)
    e = GuidedUNet(net, cu, ctx, 3.0)(x, t, down_block_additional_residuals=(du, dc), mid_block_additional_residual=(mu, mc)).sample
    e_u = net(x, t, encoder_hidden_states=cu).sample
    e_c = net(x, t, encoder_hidden_states=ctx, down_block_additional_residuals=dc, mid_block_additional_residual=mc).sample
    assert torch.equal(e, e_u + 3.0 * (e_c - e_u))
    # not the default (non-guess) guided form, where both halves carry residuals
    (gu, gc), (hu, hc) = GuidedControlNet(cnet, cu, ctx)(x, t, controlnet_cond=cond)
    assert float(gu[0].abs().max()) > 0.0
