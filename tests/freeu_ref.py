"""Reference for FreeU (Si et al. 2023; diffusers' ``apply_freeu`` / ``fourier_filter``), shared by test_freeu_cpu.py (which checks THIS
file on the CPU) and the GPU tests (which check the device path against it).  No new oracle code:

* ``fourier_filter(x, threshold, scale)`` is diffusers' function written out with ``torch.fft``: fftn over (H, W), fftshift, the block
  ``[H//2 - threshold : H//2 + threshold, W//2 - threshold : W//2 + threshold]`` times ``scale``, ifftshift, ifftn, ``.real``.
* ``direct_filter(x, scale)`` is the same map for threshold 1 without an FFT: the block holds the frequencies ky in {0, H-1}, kx in
  {0, W-1} as distinct residues, so  y = x + (s - 1) / (H W) Re(sum X(ky, kx) exp(+2 pi i (ky y / H + kx x / W))).
* ``freeu(s1, s2, b1, b2, cfg)`` swaps ``oracle.unet.resnet_block`` for a wrapper while it is active.  For ``up_blocks.{0,1}.resnets.j``
  the wrapper splits the concatenated input into hidden and skip (the skip's channels: ``cfg.skip_channels()`` reversed, stage
  q = i (layers_per_block + 1) + j), scales the first half of the hidden channels by b, filters the skip, concatenates again and calls
  the original.  Stage 0 = up block 0 takes (b1, s1), stage 1 takes (b2, s2) - diffusers' ``resolution_idx`` rule."""
import contextlib
import math
import re

import torch

SD15_DOCS = (0.9, 0.2, 1.5, 1.6)  # (s1, s2, b1, b2): the SD-1.5 values of the diffusers docs
# one parameter at a time, the others at 1: each strong enough to show at the GPU tests' tolerances (test_freeu_cpu.py asserts it)
SINGLES = {"s1": (0.2, 1.0, 1.0, 1.0), "s2": (1.0, 0.2, 1.0, 1.0), "b1": (1.0, 1.0, 1.5, 1.0), "b2": (1.0, 1.0, 1.0, 1.6)}
HW_LIST = ((1, 1), (1, 2), (3, 1), (2, 2), (2, 3), (3, 3), (4, 4), (4, 6), (5, 7), (8, 8), (16, 16))


def tiny_params():
    """The TINY UNet (+ rank-4 LoRA) of the GPU tests: (cfg, f32 state dict).  test_freeu_cpu.py measures on the same weights."""
    from oracle import unet as ou
    cfg = ou.TINY
    p = ou.init_unet_params(cfg, seed=3301, perturb_norm=True)
    p.update(ou.init_lora_params(p, rank=4, seed=3303))
    return cfg, p


def inputs(cfg, hw, seed=3310):
    """(latents [2, 4, h, w], context [2, 77, D]) of the single-forward tests."""
    g = torch.Generator().manual_seed(seed + hw[0] + hw[1])
    return torch.randn((2, 4, hw[0], hw[1]), generator=g), torch.randn((2, 77, cfg.cross_attention_dim), generator=g)


def fourier_filter(x, threshold=1, scale=1.0):
    """diffusers.utils.torch_utils.fourier_filter on [B, C, H, W], in x's own (floating) dtype."""
    B, C, H, W = x.shape
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def direct_filter(x, scale):
    """The four-coefficient form of ``fourier_filter(x, 1, scale)`` on [B, C, H, W] (float64 inside)."""
    B, C, H, W = x.shape
    xd = x.double()
    ys = torch.arange(H, dtype=torch.float64).view(H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, W)
    acc = torch.zeros_like(xd)
    for ky in sorted({0, (H - 1) % H}):
        for kx in sorted({0, (W - 1) % W}):
            ang = 2.0 * math.pi * (ky * ys / H + kx * xs / W)  # [H, W]
            fwd = torch.complex(torch.cos(ang), -torch.sin(ang))
            X = (xd.to(torch.complex128) * fwd).sum(dim=(-2, -1), keepdim=True)
            acc = acc + (X * torch.complex(torch.cos(ang), torch.sin(ang))).real
    return xd + (scale - 1.0) / (H * W) * acc


def apply_stage(hidden, skip, b, s):
    """diffusers' apply_freeu for one stage on [B, C, H, W] tensors: returns (hidden, skip)."""
    hidden = hidden.clone()
    hidden[:, :hidden.shape[1] // 2] = hidden[:, :hidden.shape[1] // 2] * b
    return hidden, fourier_filter(skip, 1, s)


_STAGE = re.compile(r"^up_blocks\.([01])\.resnets\.(\d+)$")


def stage_names(cfg):
    return [f"up_blocks.{i}.resnets.{j}" for i in range(min(2, cfg.num_levels)) for j in range(cfg.layers_per_block + 1)]


@contextlib.contextmanager
def freeu(s1, s2, b1, b2, cfg, seen=None):
    """While active, the oracle's UNet forward applies FreeU.  ``seen`` (a list) receives the names of the resnets it was applied to."""
    from oracle import unet as ou
    orig = ou.resnet_block
    rev = list(reversed(cfg.skip_channels()))
    bs = ((b1, s1), (b2, s2))

    def resnet_block(p, name, x, emb, cfg_):
        m = _STAGE.match(name)
        if m:
            i, j = int(m.group(1)), int(m.group(2))
            cs = rev[i * (cfg.layers_per_block + 1) + j]
            ch = x.shape[1] - cs
            hidden, skip = apply_stage(x[:, :ch], x[:, ch:], *bs[i])
            x = torch.cat([hidden, skip.to(x.dtype)], dim=1)
            if seen is not None:
                seen.append(name)
        return orig(p, name, x, emb, cfg_)

    ou.resnet_block = resnet_block
    try:
        yield
    finally:
        ou.resnet_block = orig
