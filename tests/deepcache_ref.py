"""Reference for the DeepCache-style feature cache (Ma et al. 2023), shared by test_deepcache_cpu.py (which checks
THIS file on the CPU) and test_gpu_deepcache.py (which checks the device code against it).  Built only from public pieces of
``oracle.unet`` - ``time_embed``, ``conv``, ``resnet_block``, ``transformer_2d``, ``_mid``, ``group_norm`` - in the order of
``oracle.unet.unet_forward``.

The encoder hands the decoder the skips s_0 .. s_{n-1} (s_0 = conv_in's output, then every resnet (+ transformer) output, then every
downsampler output).  Decoder stage q = 0 .. n-1 is one up-block resnet (+ transformer) and consumes s_{n-1-q}; upsampler convs run
between stages.  With cache depth d (1 <= d <= n-1):

  full step     the ordinary forward; the input x of stage n-1-d (the tensor concatenated with s_d, after any upsampler conv before that
                stage) is also the cache
  shallow step  time embedding, conv_in, the encoder up to and including the producer of s_d, no mid block, stages n-1-d .. n-1 with
                x = the cache (and the upsamplers between them), conv_norm_out, conv_out

s_0 .. s_d of a shallow step are exactly what the full forward would hand the decoder: a T2I-Adapter feature the full forward adds into
s_k, k <= d, is added (the in-place add into the last skip of an attention-free block too); features for deeper skips are ignored.

Schedule: with interval N, step i of a run over [first, last) is full when (i - first) % N == 0 and shallow otherwise; N = 1: no cache."""
import torch
import torch.nn.functional as F

from oracle import unet as ou


def num_skips(cfg):
    return 1 + sum(cfg.layers_per_block + (1 if i < cfg.num_levels - 1 else 0) for i in range(cfg.num_levels))


def _encoder_upto(p, cfg, x, emb, ctx, lora_scale, intrablock, last):
    """``oracle.unet._encoder`` (the in-place reading of the attention-free hand-off), stopped once s_last is final.  last = None: all."""
    skips = [x]
    feats = list(intrablock) if intrablock is not None else []
    done = lambda: last is not None and len(skips) > last  # noqa: E731
    for i in range(cfg.num_levels):
        if done():
            break
        has_attn = cfg.attn_levels[i]
        block_last = len(skips) - 1 + cfg.layers_per_block + (1 if i < cfg.num_levels - 1 else 0)  # index of this block's last skip
        for j in range(cfg.layers_per_block):
            if done():
                break
            x = ou.resnet_block(p, f"down_blocks.{i}.resnets.{j}", x, emb, cfg)
            if has_attn:
                x = ou.transformer_2d(p, f"down_blocks.{i}.attentions.{j}", x, ctx, cfg, lora_scale)
                if j == cfg.layers_per_block - 1 and feats:
                    x = x + feats.pop(0)
            skips.append(x)
        if i < cfg.num_levels - 1 and not done():
            x = ou.conv(p, f"down_blocks.{i}.downsamplers.0.conv", x, stride=2)
            skips.append(x)
        if not has_attn and feats and (last is None or last >= block_last):
            x = x + feats.pop(0)  # lands in the block's LAST skip (diffusers' in-place add): deeper than s_last when the block was cut short
            skips[-1] = x
    return x, skips


def cached_forward(p, cfg, sample, t, ctx, depth, cache=None, intrablock=None, lora_scale=1.0):
    """(eps, cache).  ``cache`` None: the full forward, returning the tensor it would store (NCHW, a clone).  ``cache`` given: the
    shallow forward from it; the cache is returned unchanged."""
    n = num_skips(cfg)
    assert 1 <= depth <= n - 1, depth
    shallow = cache is not None
    emb = ou.time_embed(p, t, sample.shape[0], cfg, sample.dtype)
    x = ou.conv(p, "conv_in", sample)
    x, skips = _encoder_upto(p, cfg, x, emb, ctx, lora_scale, intrablock, depth if shallow else None)
    if not shallow:
        x = ou._mid(p, cfg, x, emb, ctx, lora_scale)
    q, q0 = 0, n - 1 - depth
    for i in range(cfg.num_levels):
        lvl = cfg.num_levels - 1 - i
        for j in range(cfg.layers_per_block + 1):
            if shallow and q < q0:
                q += 1
                continue
            if q == q0:
                if shallow:
                    x = cache
                else:
                    cache = x.clone()
            x = torch.cat([x, skips.pop()], dim=1)
            x = ou.resnet_block(p, f"up_blocks.{i}.resnets.{j}", x, emb, cfg)
            if cfg.attn_levels[lvl]:
                x = ou.transformer_2d(p, f"up_blocks.{i}.attentions.{j}", x, ctx, cfg, lora_scale)
            q += 1
        if i < cfg.num_levels - 1 and not (shallow and q <= q0):
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = ou.conv(p, f"up_blocks.{i}.upsamplers.0.conv", x)
    x = F.silu(ou.group_norm(p, "conv_norm_out", x, cfg.norm_num_groups, cfg.norm_eps))
    return ou.conv(p, "conv_out", x), cache


class _Out:
    def __init__(self, sample):
        self.sample = sample


class CachedUNet:
    """Stateful callable with the surface of ``oracle.unet.OracleUNet``, so that the oracle's sampler loops drive it unchanged: step k
    since ``reset()`` is full when k % interval == 0 and shallow from the last full step's cache otherwise.  interval = 1: every call is
    ``oracle.unet.unet_forward``.  ``calls_per_step``: how many times the loop evaluates the network per step - 2 under
    ``guidance_ref.GuidedUNet`` (unconditional, then conditional context); every call of a step has a cache of its own, as the rows of
    the device's 2B forward have.  ``kinds`` records "full" / "shallow" per call."""

    def __init__(self, params, cfg, interval, depth, lora_scale=1.0, calls_per_step=1):
        assert interval >= 1 and 1 <= depth <= num_skips(cfg) - 1
        self.params, self.config, self.interval, self.depth, self.lora_scale = params, cfg, interval, depth, lora_scale
        self.calls_per_step = calls_per_step
        self.reset()

    def reset(self):
        self.n_calls = 0
        self.caches = [None] * self.calls_per_step
        self.kinds = []

    def eval(self):
        return self

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_intrablock_additional_residuals=None, return_dict=True):
        step, slot = divmod(self.n_calls, self.calls_per_step)
        self.n_calls += 1
        if self.interval == 1:
            self.kinds.append("full")
            y = ou.unet_forward(self.params, self.config, sample, timestep, encoder_hidden_states, down_block_additional_residuals,
                                mid_block_additional_residual, down_intrablock_additional_residuals, self.lora_scale)
            return _Out(y) if return_dict else (y,)
        assert down_block_additional_residuals is None and mid_block_additional_residual is None, "no ControlNet with a cache"
        full = step % self.interval == 0
        self.kinds.append("full" if full else "shallow")
        y, cache = cached_forward(self.params, self.config, sample, timestep, encoder_hidden_states, self.depth,
                                  None if full else self.caches[slot], down_intrablock_additional_residuals, self.lora_scale)
        self.caches[slot] = cache
        return _Out(y) if return_dict else (y,)
