"""CPU: the accepted LoRA ranks (``mrisr.check_lora_rank``), their refusal before any device work, and the algebra of the packed high-rank
layout of DESIGN.md section 18 in float64: one GEMM over K = [k | Rp] on [x | z] and [W | sB] equals x W^T + s (x A^T) B^T per module."""
import pytest
import torch

import mrisr
from oracle import unet as ou


def test_check_lora_rank_accepts_the_documented_set():
    for r in (4, 8, 12, 16, 32, 48, 64, 96, 128):
        assert mrisr.check_lora_rank(r) == r
    for r in (0, 2, 6, 20, 24, 40, 144, 256):
        with pytest.raises(ValueError, match="4, 8, 12, 16"):
            mrisr.check_lora_rank(r)
    for r in (-4, 4.0, "32", None, True):
        with pytest.raises(ValueError):
            mrisr.check_lora_rank(r)


def test_check_lora_rank_conv_stays_at_16():
    for r in (4, 8, 12, 16):
        assert mrisr.check_lora_rank(r, conv=True) == r
    for r in (32, 64, 20):
        with pytest.raises(ValueError, match="conv"):
            mrisr.check_lora_rank(r, conv=True)


def test_model_refuses_a_bad_rank_without_a_device():
    """the rank check comes before the device check: a ValueError, on a machine with or without a GPU"""
    for r in (20, 24, 144):
        with pytest.raises(ValueError, match="LoRA rank"):
            mrisr.UNet2DConditionModel(ou.TINY, compute_dtype="f32", lora_rank=r, lora_alpha=r)


def test_model_refuses_high_rank_with_fp8_naming_the_flag():
    for flag in ("fp8", "fp8_attention", "fp8_train"):
        with pytest.raises(ValueError, match=flag + ":"):
            mrisr.UNet2DConditionModel(ou.TINY, compute_dtype="bf16", lora_rank=64, lora_alpha=64, lora_fused=True, **{flag: True})


# ---- the packed layout, restated on the CPU -------------------------------------------------------------------------------------------
def _geglu_packed_rows(half):
    """mrisr.ops.geglu_packed_rows' rule: raw row g * half + j is stored at (j >> 4) * 32 + (j & 15) + 16 g"""
    j = torch.arange(half)
    p = (j >> 4) * 32 + (j & 15)
    return torch.cat([p, p + 16])


def _pack(Ws, As, Bs, s, ktile, geglu=False):
    """section 18: loraA [Rp][k] (module j's rows at j * rp, padding rows zero) and one weight [n][k + Rp]: columns [0, k) hold W, columns
    k + j * rp ... hold s B_j on the rows of module j and zero elsewhere; GEGLU: the rows in the interleave of W's rows"""
    nmod, k, r = len(Ws), Ws[0].shape[1], As[0].shape[0]
    rp = (r + ktile - 1) // ktile * ktile
    Rp = nmod * rp
    n = sum(w.shape[0] for w in Ws)
    loraA = torch.zeros(Rp, k, dtype=torch.float64)
    wt = torch.zeros(n, k + Rp, dtype=torch.float64)
    row = 0
    for j, (W, A, B) in enumerate(zip(Ws, As, Bs)):
        nj = W.shape[0]
        loraA[j * rp:j * rp + r] = A
        wt[row:row + nj, :k] = W
        wt[row:row + nj, k + j * rp:k + j * rp + r] = s * B
        row += nj
    if geglu:
        perm = _geglu_packed_rows(n // 2)
        packed = torch.empty_like(wt)
        packed[perm] = wt
        wt = packed
    return loraA, wt, rp, Rp


@pytest.mark.parametrize("r", [32, 48])
@pytest.mark.parametrize("ktile", [64, 32], ids=["bf16-tile", "f32-tile"])
def test_packed_form_equals_the_adapter_formula(r, ktile):
    g = torch.Generator().manual_seed(1800 + r + ktile)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    M, k, nj, nmod, s = 37, 40, 24, 3, 2.0
    x = rnd(M, k)
    Ws, As, Bs = [rnd(nj, k) for _ in range(nmod)], [rnd(r, k) for _ in range(nmod)], [rnd(nj, r) for _ in range(nmod)]
    loraA, wt, rp, Rp = _pack(Ws, As, Bs, s, ktile)
    assert rp % ktile == 0 and rp >= r and rp - r < ktile and wt.shape == (nmod * nj, k + Rp)
    z = x @ loraA.t()                                  # one skinny GEMM, N = Rp
    assert float(z[:, r:rp].abs().max() if rp > r else 0.0) == 0.0
    y = torch.cat([x, z], 1) @ wt.t()                  # one GEMM over K = k + Rp
    for j in range(nmod):
        want = x @ Ws[j].t() + s * (x @ As[j].t()) @ Bs[j].t()
        assert float((y[:, j * nj:(j + 1) * nj] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the backward's two banks: dz = dY (sB) on [Rp][n], dX = [dY | dz] [W | A] on [k][n + Rp]
    dY = rnd(M, nmod * nj)
    sBT = wt[:, k:].t().contiguous()                   # [Rp][n]
    dz = dY @ sBT.t()
    wd = torch.cat([wt[:, :k].t(), loraA.t()], 1)      # [k][n + Rp]
    dX = torch.cat([dY, dz], 1) @ wd.t()
    want = sum(dY[:, j * nj:(j + 1) * nj] @ (Ws[j] + s * Bs[j] @ As[j]) for j in range(nmod))
    assert float((dX - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("r", [32, 48])
def test_packed_form_geglu_interleave(r):
    g = torch.Generator().manual_seed(1900 + r)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    M, k, half, s = 19, 24, 48, 0.5
    x, W, A, B = rnd(M, k), rnd(2 * half, k), rnd(r, k), rnd(2 * half, r)
    loraA, wt, rp, Rp = _pack([W], [A], [B], s, 64, geglu=True)
    y = torch.cat([x, x @ loraA.t()], 1) @ wt.t()      # columns in the packed (value, gate) order
    want = x @ W.t() + s * (x @ A.t()) @ B.t()         # raw order: value half, then gate half
    perm = _geglu_packed_rows(half)
    assert float((y[:, perm] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    blk = y.reshape(M, half // 16, 2, 16)              # the epilogue's view: 16 values next to their 16 gates
    assert torch.equal(blk[:, :, 0].reshape(M, half), y[:, perm[:half]]) and torch.equal(blk[:, :, 1].reshape(M, half), y[:, perm[half:]])
