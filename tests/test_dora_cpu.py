"""CPU: the DoRA host surface - the reference of tests/dora_ref.py, the closed-form gradients of the contract,
``mrisr.dora_magnitude_init``, the key spellings, ``mrisr.lora_scaling``, every refusal of ``mrisr.check_dora``, and the C ABI's names.

Two tests here check the REFERENCE the GPU tests rely on rather than library code, and so do not depend on the feature:
``test_closed_form_gradients_equal_autograd_on_the_peft_forward`` (the contract's formulas, and the streaming form of dm the kernel
evaluates) and ``test_the_reference_differentiates_all_three_tensors``.  Every other test calls into ``mrisr`` and fails without it."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dora_ref as dref  # noqa: E402
import lora_ff_ref as lref  # noqa: E402
import mrisr  # noqa: E402
from mrisr.train import lora_keys_from_disk, lora_keys_to_disk  # noqa: E402
from oracle import unet as ou  # noqa: E402

MAG = ".lora_magnitude_vector.default.weight"
ALL9 = lref.ATTN + (lref.FF1, lref.FF2)


def _tiny(rank=4, seed=1900):
    cfg = ou.TINY
    up = ou.init_unet_params(cfg, seed=seed, perturb_norm=True)
    lora = lref.init_adapters(up, lref.block_modules(up, ALL9), rank, seed=seed + 1)
    return cfg, up, lora


def _batch(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((2, 4, 8, 8), generator=g), torch.randint(0, 1000, (2,), generator=g),
            torch.randn((2, 8, cfg.cross_attention_dim), generator=g))


def test_reference_at_the_initial_magnitude_is_the_lora_function():
    cfg, up, lora = _tiny()
    s = 2.0
    mags = mrisr.dora_magnitude_init(up, lora, s)
    assert set(mags) == {k[: k.index(".lora_A.")] + MAG for k in lora if ".lora_A." in k}
    x, t, ctx = _batch(cfg, 1902)
    # float64 magnitudes for the identity itself (the f32 ones of dora_magnitude_init carry their own rounding, checked below)
    m64 = {k: dref.row_norm(up[k[: -len(MAG)] + ".weight"], lora[k[: -len(MAG)] + ".lora_A.default.weight"],
                            lora[k[: -len(MAG)] + ".lora_B.default.weight"], s) for k in mags}
    with torch.no_grad():
        want = lref.forward(cfg, up, lora, s, x, t, ctx)
        got = dref.forward(cfg, up, {**lora, **m64}, s, x, t, ctx)
        got32 = dref.forward(cfg, up, {**lora, **mags}, s, x, t, ctx)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((got32 - want).norm() / want.norm()) <= 1e-6  # f32 magnitudes: g = 1 to 2^-24 per row
    for k in mags:
        assert mags[k].dtype == torch.float32 and float((mags[k].double() - m64[k]).abs().max() / m64[k].max()) <= 1e-6


@pytest.mark.parametrize("bias", [True, False])
def test_closed_form_gradients_equal_autograd_on_the_peft_forward(bias):
    g = torch.Generator().manual_seed(1910 + bias)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    M, k, n, r, s = 23, 20, 12, 4, 0.75
    x, w, a, b, dy = rnd(M, k), rnd(n, k), rnd(r, k), rnd(n, r), rnd(M, n)
    bv = rnd(n) if bias else None
    mag = torch.linalg.vector_norm(w + s * (b @ a), dim=1) * (1 + 0.1 * (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1))
    lx, la, lb, lm = (v.clone().requires_grad_(True) for v in (x, a, b, mag))
    with torch.enable_grad():
        y = dref.peft_forward(lx, w, bv, la, lb, lm, s)
        (y * dy).sum().backward()
    got = dref.closed_form_grads(x, w, bv, a, b, mag, s, dy)
    for name, gt, want in zip(("dX", "dA", "dB", "dm"), got, (lx.grad, la.grad, lb.grad, lm.grad)):
        assert float((gt - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
    # the streaming form of dm the kernel evaluates: (sum dY (Y - R) - bias sum dY) / m, with Y the epilogue's output (bias and residual in)
    res = rnd(M, n)
    yfull = y.detach() + res
    dm2 = ((dy * (yfull - res)).sum(0) - (bv if bias else 0) * dy.sum(0)) / mag
    assert float((dm2 - lm.grad).abs().max()) <= 1e-12 * float(lm.grad.abs().max())


def test_the_reference_differentiates_all_three_tensors():
    cfg, up, lora = _tiny()
    mags = dref.init_magnitudes(up, lora, 2.0, perturb=0.1, seed=3)
    x, t, ctx = _batch(cfg, 1921)
    tgt = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(1922))
    _, loss, grads = dref.loss_and_grads(cfg, up, {**lora, **mags}, 2.0, x, t, ctx, tgt)
    assert loss > 0 and set(grads) == set(lora) | set(mags)
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    # (the mid block sees ONE token at 8 x 8 latents: its self-attention softmax is constant, so q / k there get exact zeros)
    dead = ("mid_block.attentions.0.transformer_blocks.0.attn1.to_q.", "mid_block.attentions.0.transformer_blocks.0.attn1.to_k.")
    assert all(float(v.abs().max()) > 0 for k, v in grads.items() if not k.startswith(dead))


def test_magnitude_init_row_order_of_the_geglu_projection():
    cfg, up, lora = _tiny()
    s = 0.5
    mags = mrisr.dora_magnitude_init(up, lora, s)
    mod = next(k[: k.index(".lora_A.")] for k in lora if lref.FF1 + ".lora_A." in k)
    w, a, b = up[mod + ".weight"], lora[mod + ".lora_A.default.weight"], lora[mod + ".lora_B.default.weight"]
    half = w.shape[0] // 2
    m = mags[mod + MAG]
    assert m.shape == (2 * half,)
    val = torch.linalg.vector_norm(w[:half] + s * b[:half] @ a, dim=1)   # value half first
    gate = torch.linalg.vector_norm(w[half:] + s * b[half:] @ a, dim=1)  # then the gate half
    assert torch.allclose(m[:half], val, rtol=1e-6, atol=0) and torch.allclose(m[half:], gate, rtol=1e-6, atol=0)
    assert not torch.allclose(m[:half], gate, rtol=1e-3, atol=0)
    # a [c, c, 1, 1] projection (proj_in / proj_out) is a linear target too
    pin = next(k[: -len(".weight")] for k in up if k.endswith(".proj_in.weight"))
    c = up[pin + ".weight"].shape[0]
    ad = {pin + ".lora_A.default.weight": torch.randn(4, c), pin + ".lora_B.default.weight": torch.randn(c, 4)}
    assert mrisr.dora_magnitude_init(up, ad, 1.0)[pin + MAG].shape == (c,)


def test_key_round_trips_over_all_spellings():
    m = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    mem = m + MAG
    v = torch.arange(3.0)
    spellings = [mem, m + ".lora_magnitude_vector.default"]
    for pre in ("base_model.model.", "unet."):
        spellings += [pre + m + ".lora_magnitude_vector.weight", pre + m + ".lora_magnitude_vector", pre + mem]
    for k in spellings:
        assert list(lora_keys_from_disk({k: v})) == [mem], k
    assert list(lora_keys_to_disk({mem: v}, "peft")) == ["base_model.model." + m + ".lora_magnitude_vector.weight"]
    assert list(lora_keys_to_disk({mem: v}, "diffusers")) == ["unet." + m + ".lora_magnitude_vector.weight"]
    assert list(lora_keys_to_disk({mem: v}, "memory")) == [mem]
    for fmt in ("peft", "diffusers", "memory"):
        assert list(lora_keys_from_disk(lora_keys_to_disk({mem: v}, fmt))) == [mem]
    # lora_A / lora_B and foreign keys: what they were
    sd = {m + ".lora_A.default.weight": v, m + ".lora_B.default.weight": v, "conv_in.weight": v}
    assert list(lora_keys_to_disk(sd, "peft")) == ["base_model.model." + m + ".lora_A.weight", "base_model.model." + m + ".lora_B.weight",
                                                   "base_model.model.conv_in.weight"]
    assert list(lora_keys_from_disk(lora_keys_to_disk(sd, "diffusers"))) == list(sd)


def test_lora_scaling():
    assert mrisr.lora_scaling(4, 8.0) == 2.0 and mrisr.lora_scaling(16, 32) == 2.0
    assert mrisr.lora_scaling(16, 32, use_rslora=True) == 8.0
    assert mrisr.lora_scaling(64, 16, use_rslora=True) == 2.0
    assert mrisr.lora_scaling(0, 8.0) == 1.0 and mrisr.lora_scaling(4, None) == 1.0 and mrisr.lora_scaling(4, None, True) == 1.0


def _dora_sd(rank=4):
    _, up, lora = _tiny(rank)
    return up, lora, mrisr.dora_magnitude_init(up, lora, 2.0)


def test_check_dora_accepts_a_complete_state_dict_in_any_spelling():
    up, lora, mags = _dora_sd()
    mrisr.check_dora({**up, **lora, **mags}, True)
    mrisr.check_dora(lora_keys_to_disk({**lora, **mags}, "peft"), True)
    mrisr.check_dora({**up, **lora}, False)
    mrisr.check_dora({}, True)
    _, lora32, mags32 = _dora_sd(32)
    mrisr.check_dora({**lora32, **mags32}, True)


def test_check_dora_refusals():
    up, lora, mags = _dora_sd()
    full = {**up, **lora, **mags}
    for flag in ("fp8", "fp8_attention", "fp8_train"):
        with pytest.raises(ValueError, match=flag):
            mrisr.check_dora(full, True, **{flag: True})
    with pytest.raises(ValueError, match="ControlNet"):
        mrisr.check_dora(full, True, is_controlnet=True)
    with pytest.raises(ValueError, match="use_dora=True"):
        mrisr.check_dora(full, False)
    with pytest.raises(ValueError, match="use_dora=True"):  # older peft's spelling is recognised too
        mrisr.check_dora({k[: -len(".weight")]: v for k, v in mags.items()}, False)
    res = next(k[: -len(".conv1.weight")] for k in up if k.endswith(".conv1.weight"))
    conv = {res + ".conv1.lora_A.default.weight": torch.zeros(4, up[res + ".conv1.weight"].shape[1], 3, 3),
            res + ".conv1.lora_B.default.weight": torch.zeros(up[res + ".conv1.weight"].shape[0], 4, 1, 1)}
    with pytest.raises(ValueError, match="conv"):
        mrisr.check_dora({**full, **conv}, True)
    km = next(iter(mags))
    mod = km[: -len(MAG)]
    with pytest.raises(ValueError, match="without its lora_A / lora_B"):
        mrisr.check_dora({k: v for k, v in full.items() if not k.startswith(mod + ".lora_A.") and not k.startswith(mod + ".lora_B.")}, True)
    with pytest.raises(ValueError, match="without " + mod.replace(".", r"\.")):
        mrisr.check_dora({k: v for k, v in full.items() if k != km}, True)
    for bad in (torch.zeros(mags[km].shape[0] + 1), torch.zeros(mags[km].shape[0], 1), torch.zeros(())):
        with pytest.raises(ValueError, match="shape"):
            mrisr.check_dora({**full, km: bad}, True)


def test_constructors_refuse_before_any_device_work():
    """ValueError with or without a GPU: the DoRA checks come before the device check"""
    for flag in ("fp8", "fp8_attention", "fp8_train"):
        with pytest.raises(ValueError, match=flag):
            mrisr.UNet2DConditionModel(ou.TINY, compute_dtype="bf16", lora_rank=4, lora_alpha=8, use_dora=True, **{flag: True})
    with pytest.raises(ValueError, match="ControlNet"):
        mrisr.ControlNetModel(ou.TINY, compute_dtype="bf16", lora_rank=4, lora_alpha=8, use_dora=True)


def test_header_declares_the_new_entries_and_exports_list_them():
    from mrisr import _lib
    hdr = open(os.path.join(ROOT, "include", "mrisr.h")).read()
    for name in ("mrisr_model_set_dora", "mrisr_op_dora_scale", "mrisr_op_dora_mag_grad"):
        assert "int " + name + "(" in hdr and name in _lib.EXPORTS, name
