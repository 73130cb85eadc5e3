"""CPU: FreeU - the reference the GPU tests compare against (tests/freeu_ref.py: the direct four-coefficient form against the FFT form,
the identity setting against the plain oracle forward, and that every setting the GPU tests use moves the prediction by far more than
their tolerance, so that a device path with the feature silently off cannot pass there), the argument rules (``check_freeu``) and the
stage list (``freeu_stage_names``)."""
import pytest
import torch

import freeu_ref as fr

torch.set_grad_enabled(False)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12))


@pytest.mark.parametrize("hw", fr.HW_LIST, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_direct_form_equals_the_fft_form(hw):
    H, W = hw
    x = torch.randn((2, 5, H, W), dtype=torch.float64, generator=torch.Generator().manual_seed(3100 + 17 * H + W))
    for s in (0.2, 0.9, 0.0, 1.0, 2.5):
        err = float((fr.direct_filter(x, s) - fr.fourier_filter(x, 1, s)).abs().max())
        print(f"direct vs fft {H}x{W} s={s}: max abs err {err:.2e}")
        assert err <= 1e-12
    if H <= 2 and W <= 2:  # one or both frequencies of every axis are in the block: the whole plane is scaled
        assert float((fr.fourier_filter(x, 1, 0.2) - 0.2 * x).abs().max()) <= 1e-12


@pytest.fixture(scope="module")
def tiny64():
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=3101, perturb_norm=True, dtype=torch.float64)
    p.update({k: v.double() for k, v in ou.init_lora_params(p, rank=4, seed=3103).items()})
    cases = {}
    for h, w in ((8, 8), (16, 24)):
        g = torch.Generator().manual_seed(3110 + h + w)
        x = torch.randn((2, 4, h, w), dtype=torch.float64, generator=g)
        ctx = torch.randn((2, 77, cfg.cross_attention_dim), dtype=torch.float64, generator=g)
        cases[(h, w)] = (x, ctx, ou.unet_forward(p, cfg, x, torch.tensor(500), ctx))
    return cfg, p, cases


def test_identity_setting_is_the_plain_oracle_forward(tiny64):
    from oracle import unet as ou
    cfg, p, cases = tiny64
    for hw, (x, ctx, plain) in cases.items():
        seen = []
        with fr.freeu(1.0, 1.0, 1.0, 1.0, cfg, seen=seen):
            got = ou.unet_forward(p, cfg, x, torch.tensor(500), ctx)
        assert seen == fr.stage_names(cfg) and len(seen) == 6
        r = rel(got, plain)
        print(f"freeu (1,1,1,1) vs plain oracle {hw}: rel {r:.2e}")
        assert r <= 1e-12
    assert ou.resnet_block.__module__ == "oracle.unet"  # the wrapper is gone


@pytest.fixture(scope="module")
def gpu_cases():
    """The weights, inputs and sizes of test_gpu_freeu.py's single forwards."""
    from oracle import unet as ou
    cfg, p = fr.tiny_params()
    cases = {}
    for hw in ((16, 16), (16, 24)):
        x, ctx = fr.inputs(cfg, hw)
        cases[hw] = (x, ctx, ou.unet_forward(p, cfg, x, torch.tensor(500), ctx))
    return cfg, p, cases


@pytest.mark.parametrize("name", ["docs", "s1", "s2", "b1", "b2"])
def test_every_gpu_test_setting_moves_the_oracle_by_ten_f32_bounds(gpu_cases, tiny64, name):
    """The GPU tests hold the f32 engine to 1e-3: a setting that moved the prediction by less than 1e-2 could pass with FreeU off.
    Measured on the GPU tests' own weights and inputs (f32) and on the float64 cases above."""
    from oracle import unet as ou
    vals = fr.SD15_DOCS if name == "docs" else fr.SINGLES[name]
    for cfg, p, cases in (gpu_cases, tiny64):
        for hw, (x, ctx, plain) in cases.items():
            with fr.freeu(*vals, cfg):
                got = ou.unet_forward(p, cfg, x, torch.tensor(500), ctx)
            r = rel(got, plain)
            print(f"freeu {name} = {vals} on TINY {hw} {x.dtype}: relative L2 change {r:.3e}")
            assert r >= 1e-2, (name, hw, r)


def test_check_freeu_accepts_and_refuses():
    import mrisr
    chk = mrisr.check_freeu
    assert chk(0.9, 0.2, 1.5, 1.6) == (0.9, 0.2, 1.5, 1.6)
    assert chk(1, 1, 1, 1) == (1.0, 1.0, 1.0, 1.0) and all(isinstance(v, float) for v in chk(1, 1, 1, 1))
    assert chk(0, 0.0, 0, 3) == (0.0, 0.0, 0.0, 3.0)  # zero is a valid scale
    names = ("s1", "s2", "b1", "b2")
    for i, n in enumerate(names):
        for bad in (-0.1, float("nan"), float("inf"), -float("inf"), None, "x", True):
            vals = [1.0, 1.0, 1.0, 1.0]
            vals[i] = bad
            with pytest.raises(ValueError, match=rf"\b{n}\b"):
                chk(*vals)


def test_freeu_stage_names():
    import mrisr
    from oracle import unet as ou
    six = [f"up_blocks.{k}.resnets.{j}" for k in (0, 1) for j in (0, 1, 2)]
    for cfg in (ou.SD15, ou.TINY, ou.MNIST, mrisr.UNetConfig()):
        assert mrisr.freeu_stage_names(cfg) == six
    for cfg in (ou.SD15, ou.TINY, ou.MNIST):
        assert fr.stage_names(cfg) == six
    one = ou.UNetConfig(block_out_channels=(64,), attn_levels=(True,), cross_attention_dim=64)
    assert mrisr.freeu_stage_names(one) == [f"up_blocks.0.resnets.{j}" for j in (0, 1, 2)]  # a stage whose up block does not exist is skipped


def test_enable_freeu_with_a_bad_value_raises_before_touching_the_library(monkeypatch):
    import mrisr
    from mrisr import _lib

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", boom)
    net = object.__new__(mrisr.UNet2DConditionModel)  # no handle: nothing below may need one
    for vals, n in (((-1.0, 0.2, 1.5, 1.6), "s1"), ((0.9, float("nan"), 1.5, 1.6), "s2"), ((0.9, 0.2, float("inf"), 1.6), "b1"),
                    ((0.9, 0.2, 1.5, "x"), "b2")):
        with pytest.raises(ValueError, match=n):
            net.enable_freeu(*vals)
    assert net.freeu is None
