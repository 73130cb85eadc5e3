"""CPU: the host side of LoRA on ``ff.net.0.proj`` - checkpoint key forms, the row map of the GEGLU interleave, and the reference
helper tests/lora_ff_ref.py that test_gpu_lora_ff.py measures the device trainer against."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_ff_ref as ref  # noqa: E402

BLOCK = "down_blocks.0.attentions.1.transformer_blocks.0"


@pytest.mark.parametrize("key_format", ["peft", "diffusers", "memory"])
def test_ff_keys_round_trip_through_every_disk_form(key_format):
    from mrisr.train import lora_keys_from_disk, lora_keys_to_disk
    C, r = 64, 4
    sd = {f"{BLOCK}.ff.net.0.proj.lora_A.default.weight": torch.randn(r, C),
          f"{BLOCK}.ff.net.0.proj.lora_B.default.weight": torch.randn(8 * C, r),
          f"{BLOCK}.ff.net.2.lora_A.default.weight": torch.randn(r, 4 * C),
          f"{BLOCK}.ff.net.2.lora_B.default.weight": torch.randn(C, r),
          f"{BLOCK}.attn1.to_q.lora_A.default.weight": torch.randn(r, C)}
    disk = lora_keys_to_disk(sd, key_format)
    prefix = {"peft": "base_model.model.", "diffusers": "unet.", "memory": ""}[key_format]
    assert all(k.startswith(prefix) for k in disk)
    if key_format != "memory":
        assert f"{prefix}{BLOCK}.ff.net.0.proj.lora_B.weight" in disk and not any(".default." in k for k in disk)
    back = lora_keys_from_disk(disk)
    assert list(back) == list(sd) and all(back[k] is sd[k] for k in sd)
    assert lora_keys_from_disk(back).keys() == sd.keys()  # in-memory keys pass through unchanged


@pytest.mark.parametrize("half", [16, 48, 1280])
def test_geglu_row_map_is_the_packed_interleave(half):
    """raw row g * half + j (g = 0 value, 1 gate) -> packed row (j >> 4) * 32 + (j & 15) + 16 g"""
    from mrisr import ops
    perm = ops.geglu_packed_rows(half)
    assert perm.dtype == torch.int64 and perm.shape == (2 * half,)
    for g in (0, 1):
        for j in sorted({j for j in (0, 1, 15, 16, 17, half - 17, half - 16, half - 1) if 0 <= j < half}):
            assert int(perm[g * half + j]) == (j >> 4) * 32 + (j & 15) + 16 * g
    want = [(j >> 4) * 32 + (j & 15) + 16 * g for g in (0, 1) for j in range(half)]
    assert perm.tolist() == want
    assert sorted(perm.tolist()) == list(range(2 * half))            # a permutation
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(2 * half)
    assert torch.equal(inv[perm], torch.arange(2 * half)) and torch.equal(perm[inv], torch.arange(2 * half))
    # packed rows come in blocks of 16 value rows followed by their 16 gate rows
    blk = inv.reshape(-1, 2, 16)
    assert bool((blk[:, 0] < half).all()) and torch.equal(blk[:, 1], blk[:, 0] + half)
    raw = torch.randn(2 * half, 3)
    packed = torch.empty_like(raw)
    packed[perm] = raw
    assert torch.equal(packed[perm], raw)


def test_geglu_row_map_refuses_ragged_halves():
    from mrisr import ops
    for bad in (0, 8, 24, -16):
        with pytest.raises(ValueError):
            ops.geglu_packed_rows(bad)


def test_reference_helper_is_the_oracles_own_lora_forward():
    """Folding s B A into the weight is the function the oracle computes with the adapter branch, where the oracle has one (the
    attention projections); module order and count are those of the library's flat vector; gradients reach every adapter."""
    from oracle import unet as ou
    cfg = ou.UNetConfig(block_out_channels=(64, 128), attn_levels=(True, False), cross_attention_dim=64)
    up = ou.init_unet_params(cfg, seed=5, perturb_norm=True)
    mods = ref.block_modules(up, "all")
    assert len(mods) == 6 * 12 and mods[0] == "down_blocks.0.attentions.0.proj_in"
    per_block = [m.split("attentions.0.")[-1] for m in mods[:12]]
    assert per_block == ["proj_in"] + ["transformer_blocks.0." + a for a in ref.ATTN] + \
        ["transformer_blocks.0.ff.net.0.proj", "transformer_blocks.0.ff.net.2", "proj_out"]
    assert [m for m in mods if not m.endswith(ref.FF1)] == ref.block_modules(up, "existing")
    attn = ref.init_adapters(up, ref.block_modules(up, ref.ATTN), 4, seed=6)
    g = torch.Generator().manual_seed(7)
    x, ctx = torch.randn((1, 4, 8, 8), generator=g), torch.randn((1, 8, 64), generator=g)
    t = torch.tensor([371])
    with torch.no_grad():
        want = ou.unet_forward({**{k: v.double() for k, v in up.items()}, **{k: v.double() for k, v in attn.items()}}, cfg,
                               x.double(), t, ctx.double(), lora_scale=2.0)
        got = ref.forward(cfg, up, attn, 2.0, x, t, ctx)
    assert float((got - want).norm() / want.norm()) < 1e-12
    ff = ref.init_adapters(up, ref.block_modules(up, [ref.FF1])[:1], 4, seed=8)
    _, loss, grads = ref.loss_and_grads(cfg, up, ff, 2.0, x, t, ctx, torch.randn((1, 4, 8, 8), generator=g))
    (ka, a), (kb, b) = grads.items()
    assert a.shape == (4, 64) and b.shape == (512, 4) and loss > 0
    assert float(a.norm()) > 0 and float(b[:256].norm()) > 0 and float(b[256:].norm()) > 0
