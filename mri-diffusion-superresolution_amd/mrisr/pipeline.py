"""Host-side mirror of the reference's sampler glue (``src/adapters/res_srdiff.py``): same function names, argument
meaning and error behaviour; the arithmetic runs in libmrisr.so.

  get_res_shifting_latents  :7-25      prepare_condition_image :27-33
  log_validation            :35-105    decode_to_vis           :107-122

plus ``sample`` - the timestep loop itself (``:63-96``) as ONE call into the C-ABI sampler, which captures a step
(ControlNet -> UNet -> fused reverse step) into a hipGraph and replays it; no host sync on ``prev_t > 0``.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .models import ControlNetModel, UNet2DConditionModel, check_freeu, transformer_block_names


def get_res_shifting_latents(hr_latents, lr_latents, timesteps, scheduler, noise=None):
    """x_t = sqrt(a_t) HR + (1 - sqrt(a_t)) LR + sqrt(1 - a_t) eps   (reference res_srdiff.py:7-25)."""
    dev = hr_latents.device
    if noise is None:
        noise = torch.randn_like(hr_latents)
    ac = scheduler.alphas_cumprod.to(device=dev, dtype=torch.float32).contiguous()
    t = torch.as_tensor(timesteps).to(device=dev, dtype=torch.int64).contiguous()
    # the reference indexes ``alphas_cumprod[timesteps]`` and broadcasts [B,1,1,1] (:13-19): a wrong length or an index outside
    # the table is an error there; the kernel reads ac[t[b]] unchecked, so both are checked here
    if t.ndim > 1 or (t.ndim == 1 and t.numel() not in (1, hr_latents.shape[0])):
        raise RuntimeError(f"timesteps of shape {tuple(t.shape)} do not broadcast against a batch of {hr_latents.shape[0]}")
    if t.numel() and (int(t.min()) < -ac.numel() or int(t.max()) >= ac.numel()):
        raise IndexError(f"timestep out of range for an alphas_cumprod table of {ac.numel()} entries")
    if t.numel() and int(t.min()) < 0:
        t = torch.where(t < 0, t + ac.numel(), t)  # torch indexing semantics for negative indices
    hr, lr, nz = (x.to(torch.float32).contiguous() for x in (hr_latents, lr_latents, noise))
    out = torch.empty_like(hr)
    t_hr, t_lr, t_nz, t_t, t_out = (L.as_tensor(x) for x in (hr, lr, nz, t, out))
    L.check(L.lib().mrisr_resshift_forward(C.byref(t_hr), C.byref(t_lr), C.byref(t_nz), C.c_void_p(ac.data_ptr()),
                                           C.byref(t_t), C.byref(t_out), L.stream_ptr()))
    return out.to(hr_latents.dtype)


def prepare_condition_image(image, target_size=(512, 512)):
    """1 -> 3 channel expand + bilinear resize (reference res_srdiff.py:27-33).  Once per slice, outside the loop:
    tensor plumbing, done with torch on the device."""
    if image.shape[1] == 1:
        image = image.expand(-1, 3, -1, -1)
    if tuple(image.shape[-2:]) != tuple(target_size):
        image = F.interpolate(image, size=target_size, mode="bilinear", align_corners=False)
    return image


def decode_to_vis(data, vae, is_latent=True):
    """reference res_srdiff.py:107-122."""
    decoded = vae.decode(data / vae.config.scaling_factor).sample if is_latent else data
    img = (decoded / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
    img_np = (img[0] * 255).astype(np.uint8)
    if img_np.shape[-1] == 1:
        img_np = np.concatenate([img_np] * 3, axis=-1)
    return img_np


def check_guidance(guidance_scale, guidance_rescale, ehs_shape, uncond_shape, batch) -> bool:
    """The argument rules of ``Sampler.run``'s classifier-free guidance, on shapes alone (no device is touched).  Returns whether
    guidance is ACTIVE: an unconditional context is given and ``guidance_scale != 1`` (at 1 the guided prediction is the
    conditional one, so the plain call is taken).  Raises ``ValueError`` for anything a guided run could not honour."""
    g, phi = float(guidance_scale), float(guidance_rescale)
    if not np.isfinite(g):
        raise ValueError(f"guidance_scale must be finite, got {guidance_scale!r}")
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_rescale must lie in [0, 1], got {guidance_rescale!r}")
    if uncond_shape is None:
        if g != 1.0:
            raise ValueError("guidance_scale != 1 needs uncond_hidden_states (the embedding of the empty caption)")
        if phi > 0.0:
            raise ValueError("guidance_rescale > 0 needs active guidance: uncond_hidden_states and guidance_scale != 1")
        return False
    ehs_shape, uncond_shape = tuple(ehs_shape), tuple(uncond_shape)
    if len(ehs_shape) != 3 or ehs_shape[0] not in (1, batch):
        raise ValueError(f"encoder_hidden_states must be [1, L, D] or [{batch}, L, D], got {ehs_shape}")
    if len(uncond_shape) != 3 or uncond_shape[0] not in (1, batch) or uncond_shape[1:] != ehs_shape[1:]:
        raise ValueError(f"uncond_hidden_states must be [1, L, D] or [{batch}, L, D] with the L and D of encoder_hidden_states "
                         f"{ehs_shape}, got {uncond_shape}")
    if g == 1.0:
        if phi > 0.0:
            raise ValueError("guidance_rescale > 0 needs active guidance: guidance_scale != 1")
        return False
    return True


def check_pag(pag_scale, applied_layers, block_names, has_cache=False, fp8_attention=False) -> int:
    """The argument rules of perturbed-attention guidance (``Sampler.run(pag_scale=, pag_applied_layers=)``), on
    numbers and names alone (no device is touched).  Returns the block mask - bit i = ``block_names[i]``, the UNet's transformer blocks
    in forward order (``transformer_block_names``) - or 0 when ``pag_scale == 0``: PAG off, the plain call is taken.

    ``applied_layers``: a prefix or a tuple of prefixes; a prefix selects every block whose name starts with it at a component
    boundary (``"mid"`` stands for ``"mid_block"``; ``"down_blocks.2"``, ``"up_blocks.1.attentions.0"``).  Raises ``ValueError`` naming
    the argument: ``pag_scale`` negative or not finite; an entry that selects nothing; with ``pag_scale > 0`` an empty tuple, a feature
    cache with interval > 1 (its shallow pass skips the blocks PAG perturbs) or a UNet built with ``fp8_attention``."""
    try:
        s = float(pag_scale)
    except (TypeError, ValueError):
        raise ValueError(f"pag_scale must be a number >= 0, got {pag_scale!r}") from None
    if isinstance(pag_scale, bool) or not np.isfinite(s) or s < 0.0:
        raise ValueError(f"pag_scale must be finite and >= 0, got {pag_scale!r}")
    layers = (applied_layers,) if isinstance(applied_layers, str) else tuple(applied_layers if applied_layers is not None else ())
    names = list(block_names)
    mask = 0
    for entry in layers:
        if not isinstance(entry, str) or not entry:
            raise ValueError(f"pag_applied_layers: every entry must be a non-empty string, got {entry!r}")
        parts = entry.split(".")
        if parts[0] == "mid":
            parts[0] = "mid_block"
        hit = [i for i, n in enumerate(names) if n.split(".")[:len(parts)] == parts]
        if not hit:
            raise ValueError(f"pag_applied_layers: {entry!r} selects no transformer block; the blocks are {', '.join(names)}")
        for i in hit:
            mask |= 1 << i
    if s == 0.0:
        return 0
    if len(names) > 32:
        raise ValueError(f"pag_scale > 0: at most 32 transformer blocks fit the block mask, the UNet has {len(names)}")
    if not layers:
        raise ValueError("pag_applied_layers must name at least one block when pag_scale > 0")
    if has_cache:
        raise ValueError("pag_scale > 0 together with a feature cache (cache interval > 1) is not supported: the shallow pass skips the "
                         "blocks PAG perturbs")
    if fp8_attention:
        raise ValueError("pag_scale > 0 is not supported on a UNet built with fp8_attention")
    return mask


NEUTRAL_ROW = (1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0)  # the guided prediction is the conditional one, FreeU the identity
SCHEDULE_COLUMNS = ("guidance_scale", "pag_scale", "guidance_rescale", "freeu_s1", "freeu_s2", "freeu_b1", "freeu_b2", "padding")
FULL_INTERVAL = (0.0, 1.0)


def _check_interval(name, interval):
    try:
        lo, hi = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a (start, end) pair of numbers, got {interval!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)) or not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"{name} must satisfy 0 <= start <= end <= 1, got {interval!r}")
    return lo, hi


def _finite(name, v, lo=None):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, got {v!r}") from None
    if isinstance(v, bool) or not np.isfinite(f):
        raise ValueError(f"{name} must be finite, got {v!r}")
    if lo is not None and f < lo:
        raise ValueError(f"{name} must be >= {lo:g}, got {v!r}")
    return f


def check_schedule(schedule, n_steps) -> np.ndarray:
    """The rules of an explicit schedule table (``Sampler.run(schedule=)``), on numbers alone (no device is
    touched): ``[n_steps, 8]`` rows ``{g, s, phi, freeu_s1, freeu_s2, freeu_b1, freeu_b2, 0}``, every value finite, ``s >= 0``,
    ``0 <= phi <= 1``, the FreeU values ``>= 0``.  Returns it as a contiguous float32 array; raises ``ValueError`` naming the column."""
    try:
        a = np.ascontiguousarray(np.asarray(schedule, dtype=np.float32))
    except (TypeError, ValueError):
        raise ValueError("schedule must be an array of numbers") from None
    if a.ndim != 2 or a.shape != (int(n_steps), 8):
        raise ValueError(f"schedule must have shape [{int(n_steps)}, 8] (one row per step of the sampler), got {list(a.shape)}")
    for c, name in enumerate(SCHEDULE_COLUMNS):
        col = a[:, c]
        if not np.isfinite(col).all():
            raise ValueError(f"schedule: column {c} ({name}) holds a value that is not finite")
        if c == 1 and (col < 0).any():
            raise ValueError("schedule: column 1 (pag_scale) must be >= 0")
        if c == 2 and ((col < 0) | (col > 1)).any():
            raise ValueError("schedule: column 2 (guidance_rescale) must lie in [0, 1]")
        if 3 <= c <= 6 and (col < 0).any():
            raise ValueError(f"schedule: column {c} ({name}) must be >= 0")
    return a


def step_schedule(timesteps, guidance_scale=1.0, guidance_rescale=0.0, pag_scale=0.0, pag_adaptive_scale=0.0,
                  guidance_interval=FULL_INTERVAL, pag_interval=FULL_INTERVAL, freeu=None, freeu_interval=FULL_INTERVAL,
                  num_train_timesteps=1000) -> np.ndarray:
    """The per-step schedule table of ``Sampler.run(schedule=)`` for the ``n`` steps at ``timesteps``: float32
    ``[n, 8]``, row i = ``{g, s, phi, freeu_s1, freeu_s2, freeu_b1, freeu_b2, 0}`` of step i.  Pure Python on the CPU.  The rules:

    * Adaptive PAG: ``s_i = max(pag_scale - pag_adaptive_scale * (num_train_timesteps - t_i), 0)`` - the rule of diffusers' PAG mixin
      with its 1000 generalised (diffusers is not available to this project: the formula is the specification).  The scale decays
      from the high-noise end and is clamped at 0.
    * Intervals: step i of n is inside ``(lo, hi)`` iff ``i / n >= lo and (i + 1) / n <= hi`` - diffusers' ``control_guidance_start`` /
      ``control_guidance_end`` rule; ``0 <= lo <= hi <= 1``.  Outside ``guidance_interval``: ``g = 1``.  Outside ``pag_interval``:
      ``s = 0``.  Outside ``freeu_interval`` (or with ``freeu=None``): ``(1, 1, 1, 1)``; inside, the ``freeu = (s1, s2, b1, b2)`` values.
    * A row with ``g == 1`` and ``s == 0`` gets ``phi = 0``: there is nothing to rescale, the prediction is the conditional one.
    * So a step outside every interval is the neutral row ``{1, 0, 0, 1, 1, 1, 1, 0}``.

    Raises ``ValueError`` for a value that is not finite, ``pag_scale`` or ``pag_adaptive_scale`` < 0, ``guidance_rescale`` outside
    [0, 1], a negative FreeU value, a timestep outside ``[0, num_train_timesteps)`` or an interval that breaks the rule above."""
    ts = np.asarray(timesteps.detach().cpu().numpy() if isinstance(timesteps, torch.Tensor) else timesteps)
    if ts.ndim != 1 or ts.size == 0 or not np.isfinite(ts.astype(np.float64)).all():
        raise ValueError("timesteps must be a non-empty 1-D sequence of finite numbers")
    T = int(num_train_timesteps)
    if T < 1 or (ts < 0).any() or (ts >= T).any():
        raise ValueError(f"timesteps must lie in [0, num_train_timesteps = {num_train_timesteps!r})")
    g = _finite("guidance_scale", guidance_scale)
    phi = _finite("guidance_rescale", guidance_rescale, 0.0)
    if phi > 1.0:
        raise ValueError(f"guidance_rescale must lie in [0, 1], got {guidance_rescale!r}")
    s0 = _finite("pag_scale", pag_scale, 0.0)
    ad = _finite("pag_adaptive_scale", pag_adaptive_scale, 0.0)
    g_iv, p_iv, f_iv = (_check_interval(n, v) for n, v in (("guidance_interval", guidance_interval), ("pag_interval", pag_interval),
                                                            ("freeu_interval", freeu_interval)))
    fu = None
    if freeu is not None:
        if len(tuple(freeu)) != 4:
            raise ValueError(f"freeu must be a (s1, s2, b1, b2) tuple, got {freeu!r}")
        fu = tuple(check_freeu(*freeu))
    n = int(ts.size)

    def inside(i, iv):
        return i / n >= iv[0] and (i + 1) / n <= iv[1]

    rows = np.empty((n, 8), dtype=np.float32)
    for i in range(n):
        gi = g if inside(i, g_iv) else 1.0
        si = max(s0 - ad * (T - float(ts[i])), 0.0) if inside(i, p_iv) else 0.0
        si = float(np.float32(si))
        pi = 0.0 if (float(np.float32(gi)) == 1.0 and si == 0.0) else phi
        with np.errstate(over="ignore"):
            rows[i] = (gi, si, pi) + (fu if fu is not None and inside(i, f_iv) else (1.0, 1.0, 1.0, 1.0)) + (0.0,)
    if not np.isfinite(rows).all():
        raise ValueError("a value of the schedule is not finite in float32")
    return rows


CONDITIONING_COLUMNS = ("controlnet_conditioning_scale", "adapter_conditioning_scale", "padding", "padding")


def check_conditioning(table, n_steps) -> np.ndarray:
    """The rules of an explicit conditioning table (``Sampler.run(conditioning=)``), on numbers alone (no device is
    touched): ``[n_steps, 4]`` rows ``{c, a, 0, 0}``, every value finite, columns 2 and 3 zero.  Returns it as a contiguous float32
    array; raises ``ValueError`` naming the column."""
    try:
        a = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    except (TypeError, ValueError):
        raise ValueError("conditioning must be an array of numbers") from None
    if a.ndim != 2 or a.shape != (int(n_steps), 4):
        raise ValueError(f"conditioning must have shape [{int(n_steps)}, 4] (one row per step of the sampler), got {list(a.shape)}")
    for c, name in enumerate(CONDITIONING_COLUMNS):
        if not np.isfinite(a[:, c]).all():
            raise ValueError(f"conditioning: column {c} ({name}) holds a value that is not finite")
        if c >= 2 and (a[:, c] != 0).any():
            raise ValueError(f"conditioning: column {c} ({name}) must be 0")
    return a


def conditioning_schedule(n_steps, controlnet_conditioning_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0,
                          adapter_conditioning_scale=1.0, adapter_conditioning_factor=1.0) -> np.ndarray:
    """The conditioning table of ``Sampler.run(conditioning=)`` for a run of ``n_steps`` steps: float32
    ``[n_steps, 4]``, row i = ``{c_i, a_i, 0, 0}``.  Pure Python on the CPU.  The rules (diffusers is not available to this project: the
    formulae are the specification):

    * ``c_i = controlnet_conditioning_scale`` if step i is inside ``(control_guidance_start, control_guidance_end)`` - that is,
      ``i / n >= start and (i + 1) / n <= end``, diffusers' ``controlnet_keep`` and the ``inside`` rule of ``step_schedule`` - and 0 otherwise.
    * ``a_i = adapter_conditioning_scale`` if ``i < int(n * adapter_conditioning_factor)`` - the rule of diffusers' T2I-Adapter
      pipeline - and 0 otherwise.
    * So the defaults give the neutral row ``{1, 1, 0, 0}`` on every step.

    Raises ``ValueError`` for ``n_steps < 1``, a value that is not finite (also once rounded to float32), ``start`` / ``end`` that break
    ``0 <= start <= end <= 1`` or a factor outside [0, 1]."""
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
        raise ValueError(f"n_steps must be an int >= 1, got {n_steps!r}")
    n = int(n_steps)
    c = _finite("controlnet_conditioning_scale", controlnet_conditioning_scale)
    a = _finite("adapter_conditioning_scale", adapter_conditioning_scale)
    lo, hi = _check_interval("(control_guidance_start, control_guidance_end)", (control_guidance_start, control_guidance_end))
    fac = _finite("adapter_conditioning_factor", adapter_conditioning_factor, 0.0)
    if fac > 1.0:
        raise ValueError(f"adapter_conditioning_factor must lie in [0, 1], got {adapter_conditioning_factor!r}")
    rows = np.zeros((n, 4), dtype=np.float32)
    with np.errstate(over="ignore"):
        for i in range(n):
            rows[i, 0] = c if (i / n >= lo and (i + 1) / n <= hi) else 0.0
            rows[i, 1] = a if i < int(n * fac) else 0.0
    if not np.isfinite(rows).all():
        raise ValueError("a value of the conditioning table is not finite in float32")
    return rows


CONSISTENCY_FILTERS = dict(L.CONSISTENCY_FILTERS)
CONSISTENCY_COLUMNS = ("weight", "alpha", "beta", "sigma")
CONSISTENCY_LDS_CAP = 65536
SAMPLER_KINDS = ("ddim", "resshift", "ddpm", "unipc", "dpmsolver++")


def check_consistency(factor, filter, h, w, cache_interval=1):
    """The argument rules of low-frequency consistency (``Sampler.run(consistency_ref=)``), on numbers alone (no
    device is touched); returns the normalised (factor, filter id).  ``factor`` N: an int in 2..8 that divides ``h`` and ``w`` of the
    latent canvas; ``filter``: "bilinear" or "nearest"; the canvas must fit the kernel's LDS scratch, ``4 (h w / N + h w / N^2)`` bytes
    <= 64 KB (128 x 128 latents at N = 2 need 48 KB; 256 x 256 needs N >= 8); a feature cache (``cache_interval`` > 1) is refused.
    Raises ``ValueError`` naming the argument."""
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 2 <= factor <= 8:
        raise ValueError(f"consistency_factor must be an int in 2..8, got {factor!r}")
    if not isinstance(filter, str) or filter not in CONSISTENCY_FILTERS:
        raise ValueError(f"consistency_filter must be one of {tuple(CONSISTENCY_FILTERS)}, got {filter!r}")
    for name, v in (("h", h), ("w", w)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} of the latents must be an int >= 1, got {v!r}")
    N, h, w = int(factor), int(h), int(w)
    if h % N or w % N:
        raise ValueError(f"consistency_factor {N} must divide h and w of the latents, got {h} x {w}")
    need = 4 * (h * (w // N) + (h // N) * (w // N))
    if need > CONSISTENCY_LDS_CAP:
        raise ValueError(f"consistency_factor {N} on {h} x {w} latents needs {need} bytes of LDS, more than {CONSISTENCY_LDS_CAP}: use a "
                         "larger consistency_factor")
    if cache_interval > 1:
        raise ValueError("consistency_ref together with a feature cache (interval > 1) is not supported")
    return N, CONSISTENCY_FILTERS[filter]


def check_consistency_table(table, n_steps) -> np.ndarray:
    """The rules of an explicit consistency table (``Sampler.run(consistency=)``), on numbers alone (no device is
    touched): ``[n_steps, 4]`` rows ``{w, alpha, beta, sigma}``, every value finite.  Returns it as a contiguous float32 array; raises
    ``ValueError`` naming the column."""
    try:
        with np.errstate(over="ignore"):  # (a value too large for float32 becomes inf and is named below)
            a = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    except (TypeError, ValueError):
        raise ValueError("consistency must be an array of numbers") from None
    if a.ndim != 2 or a.shape != (int(n_steps), 4):
        raise ValueError(f"consistency must have shape [{int(n_steps)}, 4] (one row per step of the sampler), got {list(a.shape)}")
    for c, name in enumerate(CONSISTENCY_COLUMNS):
        if not np.isfinite(a[:, c]).all():
            raise ValueError(f"consistency: column {c} ({name}) holds a value that is not finite")
    return a


def consistency_schedule(timesteps, alphas_cumprod, kind, anchored, weight=1.0, interval=FULL_INTERVAL, noisy=False,
                         final_sigmas_type="zero") -> np.ndarray:
    """The consistency table of ``Sampler.run(consistency=)`` for the ``n`` steps at ``timesteps``: float32
    ``[n, 4]``, row i = ``{w_i, alpha_i, beta_i, sigma_i}``.  Pure Python on the CPU.  After step i the state is pulled towards
    ``y_i = alpha_i ref + beta_i lr + sigma_i z_i``: the reference at the noise level of the state step i PRODUCES.  With ``a_p(i)`` the
    cumulative alpha of that state - ``alphas_cumprod[timesteps[i + 1]]``, and for the last step the point the step rule of ``kind`` lands
    on: 1 for "ddpm" and for the multistep kinds with ``final_sigmas_type="zero"``, ``alphas_cumprod[0]`` for "ddim", "resshift" and
    "sigma_min" -

    * ``alpha_i = sqrt(a_p)``;
    * ``beta_i = 1 - sqrt(a_p)`` when ``anchored`` (the mean of the shift process: "resshift" always, any other kind run with
      ``lr_latents``), else 0;
    * ``sigma_i = sqrt(1 - a_p)`` when ``noisy`` (ILVR's noised reference; the run then needs ``consistency_noise``), else 0;
    * ``w_i = weight`` when step i is inside ``interval`` (``i / n >= start and (i + 1) / n <= end``, the rule of ``step_schedule``), else 0.

    Raises ``ValueError`` for an unknown ``kind`` or ``final_sigmas_type``, values that are not finite, ``weight`` < 0, a timestep outside
    the table or an interval that breaks ``0 <= start <= end <= 1``."""
    if kind not in SAMPLER_KINDS:
        raise ValueError(f"kind must be one of {SAMPLER_KINDS}, got {kind!r}")
    if final_sigmas_type not in ("zero", "sigma_min"):
        raise ValueError(f"final_sigmas_type must be 'zero' or 'sigma_min', got {final_sigmas_type!r}")
    ts = np.asarray(timesteps.detach().cpu().numpy() if isinstance(timesteps, torch.Tensor) else timesteps)
    if ts.ndim != 1 or ts.size == 0 or not np.isfinite(ts.astype(np.float64)).all():
        raise ValueError("timesteps must be a non-empty 1-D sequence of finite numbers")
    ac = np.asarray(alphas_cumprod.detach().cpu().numpy() if isinstance(alphas_cumprod, torch.Tensor) else alphas_cumprod, dtype=np.float64)
    if ac.ndim != 1 or ac.size == 0 or not np.isfinite(ac).all() or (ac < 0).any() or (ac > 1).any():
        raise ValueError("alphas_cumprod must be a non-empty 1-D table of finite values in [0, 1]")
    if (ts < 0).any() or (ts >= ac.size).any():
        raise ValueError(f"timesteps must lie in [0, {ac.size}): the alphas_cumprod table")
    wgt = _finite("weight", weight, 0.0)
    lo, hi = _check_interval("interval", interval)
    n = int(ts.size)
    if kind == "ddpm" or (kind in MULTISTEP_KINDS and final_sigmas_type == "zero"):
        a_last = 1.0
    else:
        a_last = float(ac[0])
    rows = np.zeros((n, 4), dtype=np.float32)
    with np.errstate(over="ignore"):
        for i in range(n):
            a_p = float(ac[int(ts[i + 1])]) if i + 1 < n else a_last
            rows[i] = (wgt if (i / n >= lo and (i + 1) / n <= hi) else 0.0, np.sqrt(a_p), 1.0 - np.sqrt(a_p) if anchored else 0.0,
                       np.sqrt(1.0 - a_p) if noisy else 0.0)
    if not np.isfinite(rows).all():
        raise ValueError("a value of the consistency table is not finite in float32")
    return rows


STEP_REDUCED, STEP_NO_CONTROLNET, STEP_NO_FEATURES = 1, 2, 4


def step_variants(schedule, conditioning, K, has_controlnet=False, n_features=0, pag=False, n_steps=None) -> List[int]:
    """What each step of a run with ``Sampler.run(skip_neutral=True)`` leaves out: one small int per step, a
    sum of ``STEP_REDUCED`` (1), ``STEP_NO_CONTROLNET`` (2) and ``STEP_NO_FEATURES`` (4); 0 is the full step.  Pure Python on the CPU;
    the library applies the same rule to the same float32 rows.  Row i belongs to step i of the schedule, also under ``set_range``.

    * ``schedule``: the run's ``[n, 8]`` table (``check_schedule``) or None.  ``K``: the parts of the forward - 1 plain, 2 classifier-free
      guidance or PAG alone (``pag=True``), 3 both.  With a table and ``K`` > 1, a row with ``g == 1`` and ``s == 0`` - PAG alone:
      ``s == 0`` - is **reduced**: its guided prediction is the conditional one, so the forward runs on the B conditional rows only.
      ``phi`` does not matter (the rescale factor of a prediction against itself is 1); ``-0.0`` counts as 0.
    * ``conditioning``: the run's ``[n, 4]`` table (``check_conditioning``) or None.  With a ControlNet, a row with ``c == 0`` runs
      **no ControlNet**; with ``n_features`` > 0, a row with ``a == 0`` takes **no adapter features**.
    * A run without the relevant table, or without the network a column speaks of, has nothing to skip there.  FreeU is not part of a
      variant.  With neither table the answer is ``n_steps`` zeros.

    Raises ``ValueError`` for ``K`` outside 1..3, ``pag`` with ``K`` == 1, tables of different lengths or no length at all."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= 3:
        raise ValueError(f"K must be 1, 2 or 3, got {K!r}")
    if pag and K == 1:
        raise ValueError("pag=True needs K = 2 (PAG alone) or 3 (with classifier-free guidance)")
    if isinstance(n_features, bool) or not isinstance(n_features, (int, np.integer)) or n_features < 0:
        raise ValueError(f"n_features must be an int >= 0, got {n_features!r}")
    lengths = set()
    if schedule is not None:
        schedule = np.asarray(schedule, dtype=np.float32)
        if schedule.ndim != 2 or schedule.shape[1] != 8:
            raise ValueError(f"schedule must have shape [n, 8], got {list(schedule.shape)}")
        lengths.add(int(schedule.shape[0]))
    if conditioning is not None:
        conditioning = np.asarray(conditioning, dtype=np.float32)
        if conditioning.ndim != 2 or conditioning.shape[1] != 4:
            raise ValueError(f"conditioning must have shape [n, 4], got {list(conditioning.shape)}")
        lengths.add(int(conditioning.shape[0]))
    if n_steps is not None:
        lengths.add(int(n_steps))
    if len(lengths) != 1:
        raise ValueError("the tables (and n_steps) must agree on one number of steps" if lengths else
                         "without a table the number of steps must be given (n_steps)")
    n = lengths.pop()
    out = []
    for i in range(n):
        v = 0
        if schedule is not None and K > 1:
            g, s = schedule[i, 0], schedule[i, 1]
            if s == 0 and ((pag and K == 2) or g == 1):
                v |= STEP_REDUCED
        if conditioning is not None:
            if has_controlnet and conditioning[i, 0] == 0:
                v |= STEP_NO_CONTROLNET
            if n_features > 0 and conditioning[i, 1] == 0:
                v |= STEP_NO_FEATURES
        out.append(v)
    return out


def check_skip(skip_neutral, cache_interval=1) -> bool:
    """The argument rule of ``Sampler.run(skip_neutral=)`` (no device is touched): a bool; True is refused together with a feature cache
    (``cache_interval`` > 1), whose shallow step has no reduced form.  Raises ``ValueError``."""
    if not isinstance(skip_neutral, (bool, np.bool_)):
        raise ValueError(f"skip_neutral must be a bool, got {skip_neutral!r}")
    if skip_neutral and cache_interval > 1:
        raise ValueError("skip_neutral=True together with a feature cache (interval > 1) is not supported")
    return bool(skip_neutral)


def guess_mode_weights(n_down) -> np.ndarray:
    """The per-residual weights of guess mode (diffusers' ``ControlNetModel.forward``): float32 ``logspace(-1, 0, n_down + 1)`` - the
    ``n_down`` down residuals, then the mid residual at weight 1."""
    if isinstance(n_down, bool) or not isinstance(n_down, (int, np.integer)) or n_down < 0:
        raise ValueError(f"n_down must be an int >= 0, got {n_down!r}")
    w = np.logspace(-1.0, 0.0, int(n_down) + 1).astype(np.float32)
    w[-1] = 1.0
    return w


MULTISTEP_KINDS = ("unipc", "dpmsolver++")


def check_solver(kind, solver_order=2, final_sigmas_type="zero", lower_order_final=True, disable_corrector=()):
    """The argument rules of the multistep sampler kinds (no device is touched); returns the normalised
    (solver_order, final_sigmas_type, disable_corrector).  Raises ``ValueError`` for anything the solver could not honour."""
    if kind not in MULTISTEP_KINDS:
        raise ValueError(f"solver must be one of {MULTISTEP_KINDS}, got {kind!r}")
    top = 3 if kind == "unipc" else 2
    if isinstance(solver_order, bool) or not isinstance(solver_order, (int, np.integer)) or not 1 <= solver_order <= top:
        raise ValueError(f"solver_order must be 1..{top} for {kind}, got {solver_order!r}")
    if final_sigmas_type not in ("zero", "sigma_min"):
        raise ValueError(f"final_sigmas_type must be 'zero' or 'sigma_min', got {final_sigmas_type!r}")
    if lower_order_final is not True:
        raise ValueError("lower_order_final=False is not implemented")
    disable = [int(i) for i in (disable_corrector or ())]
    if disable and kind != "unipc":
        raise ValueError("disable_corrector belongs to UniPC")
    if any(i < 0 for i in disable):
        raise ValueError("disable_corrector: step indices must be >= 0")
    return int(solver_order), final_sigmas_type, disable


def check_cache(interval, depth, n_skips, has_controlnet=False):
    """The argument rules of the sampler's feature cache (``Sampler.set_cache``), on numbers alone (no device is touched); returns
    the normalised (interval, depth).  ``interval`` >= 1 (1: no cache); 1 <= ``depth`` <= ``n_skips`` - 1; a ControlNet together
    with ``interval`` > 1 is refused (its shallow pass does not exist).  Raises ``ValueError``."""
    for name, v in (("interval", interval), ("depth", depth)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"cache {name} must be an int, got {v!r}")
    if interval < 1:
        raise ValueError(f"cache interval must be >= 1 (1: no cache), got {interval}")
    if not 1 <= depth <= n_skips - 1:
        raise ValueError(f"cache depth must lie in 1..{n_skips - 1}, got {depth}")
    if interval > 1 and has_controlnet:
        raise ValueError("a feature cache (interval > 1) together with a ControlNet is not supported")
    return int(interval), int(depth)


TILE_WINDOWS = tuple(L.TILE_WINDOWS)


def check_tiles(tile, overlap, window, divisor, has_cache=False):
    """The argument rules of tiled sampling (``Sampler.set_tiles``), on numbers alone (no device is touched); returns the normalised
    (t_h, t_w, o_h, o_w, window).  ``tile`` / ``overlap``: an int or a (h, w) pair, in latent pixels, multiples of ``divisor``
    (the UNet's own rule for h and w, 2^(levels-1)); tile >= divisor; 0 <= overlap < tile; ``window`` "gaussian" or "uniform"; a
    feature cache together with tiles is refused.  Raises ``ValueError`` naming the offending argument."""
    def pair(name, v):
        vs = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        if len(vs) != 2 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in vs):
            raise ValueError(f"{name} must be an int or a pair of ints (h, w), got {v!r}")
        return int(vs[0]), int(vs[1])

    d = int(divisor)
    t_h, t_w = pair("tile", tile)
    o_h, o_w = pair("overlap", overlap)
    for t in (t_h, t_w):
        if t < d or t % d:
            raise ValueError(f"tile must be a multiple of {d} (latent pixels) and at least {d}, got {tile!r}")
    for t, o in ((t_h, o_h), (t_w, o_w)):
        if o < 0 or o >= t or o % d:
            raise ValueError(f"overlap must be a multiple of {d} in 0 .. tile - 1, got {overlap!r} for tile {tile!r}")
    if window not in TILE_WINDOWS:
        raise ValueError(f"window must be one of {TILE_WINDOWS}, got {window!r}")
    if has_cache:
        raise ValueError("tiles together with a feature cache (cache interval > 1) are not supported")
    return t_h, t_w, o_h, o_w, window


def tile_tables(extent, tile, overlap, window="gaussian"):
    """One axis of the tile grid and its blend window, from the library's own host routine (``mrisr_tile_tables``; no GPU):
    (origins: list[int], weights: f32 tensor [n_tiles, min(tile, extent)]), the weights normalised over the covering tiles."""
    if window not in TILE_WINDOWS:
        raise ValueError(f"window must be one of {TILE_WINDOWS}, got {window!r}")
    lib, wid = L.lib(), L.TILE_WINDOWS[window]
    k = C.c_int(0)
    L.check(lib.mrisr_tile_tables(int(extent), int(tile), int(overlap), wid, None, None, C.byref(k)))
    origins = (C.c_int * k.value)()
    weights = torch.empty((k.value, min(int(tile), int(extent))), dtype=torch.float32)
    L.check(lib.mrisr_tile_tables(int(extent), int(tile), int(overlap), wid, origins, C.c_void_p(weights.data_ptr()), C.byref(k)))
    return list(origins), weights


def _tile_crops(x, ys, xs, s_h, s_w):
    """[N, C, H, W] -> [N*T, C, s_h, s_w]: the crop at every (y, x) of ys x xs (y-major) of every row, sample-major."""
    crops = [x[..., y:y + s_h, xx:xx + s_w] for y in ys for xx in xs]
    return torch.stack(crops, dim=1).flatten(0, 1).contiguous()


def _build_schedule(n_steps, timesteps, n_train, freeu, schedule, pag_adaptive_scale, guidance_interval, pag_interval, freeu_interval, g, phi,
                    pag_scale, pag_on, has_uncond):
    """The schedule table of a ``Sampler.run`` (float32 [n_steps, 8]) or None: no table, the call of before.  ``timesteps`` / ``n_train``:
    the sampler's grid; ``freeu``: the UNet's ``enable_freeu`` state or None.  Everything is checked here, before anything is launched."""
    ad = _finite("pag_adaptive_scale", pag_adaptive_scale, 0.0)
    ivs = {"guidance_interval": guidance_interval, "pag_interval": pag_interval, "freeu_interval": freeu_interval}
    ivs = {k: (FULL_INTERVAL if v is None else _check_interval(k, v)) for k, v in ivs.items()}
    given = [k for k, v in ivs.items() if v != FULL_INTERVAL] + (["pag_adaptive_scale"] if ad > 0.0 else [])
    if schedule is not None:
        if given:
            raise ValueError(f"schedule is an explicit table: it excludes {', '.join(given)}")
        return check_schedule(schedule, n_steps)
    if not given:
        return None
    if (ad > 0.0 or ivs["pag_interval"] != FULL_INTERVAL) and not pag_on:
        raise ValueError("pag_adaptive_scale / pag_interval need perturbed-attention guidance: pag_scale > 0")
    if ivs["guidance_interval"] != FULL_INTERVAL and not (has_uncond and float(g) != 1.0):
        raise ValueError("guidance_interval needs active classifier-free guidance: uncond_hidden_states and guidance_scale != 1")
    if ivs["freeu_interval"] != FULL_INTERVAL and freeu is None:
        raise ValueError("freeu_interval needs FreeU on the UNet (unet.enable_freeu): it schedules that state's four values")
    return step_schedule(timesteps, guidance_scale=g if has_uncond else 1.0, guidance_rescale=phi, pag_scale=pag_scale,
                         pag_adaptive_scale=ad, guidance_interval=ivs["guidance_interval"], pag_interval=ivs["pag_interval"],
                         freeu=freeu, freeu_interval=ivs["freeu_interval"], num_train_timesteps=n_train)


def _build_conditioning(n_steps, has_controlnet, tiles_on, cache_interval, conditioning, c_scale, start, end, a_scale, factor, guess_mode,
                        pag_on, has_features):
    """(table, guess) of a ``Sampler.run`` - float32 [n_steps, 4] and a bool - or None: no table, the call of before.  Everything is
    checked here, before anything is launched."""
    named = {"controlnet_conditioning_scale": (c_scale, 1.0), "control_guidance_start": (start, 0.0),
             "control_guidance_end": (end, 1.0), "adapter_conditioning_scale": (a_scale, 1.0),
             "adapter_conditioning_factor": (factor, 1.0)}
    given = [k for k, (v, d) in named.items() if _finite(k, v) != d]
    guess = bool(guess_mode)
    if conditioning is not None:
        if given:
            raise ValueError(f"conditioning is an explicit table: it excludes {', '.join(given)}")
        table = check_conditioning(conditioning, n_steps)
    elif given or guess:
        table = conditioning_schedule(n_steps, c_scale, start, end, a_scale, factor)
    else:
        return None
    if not has_controlnet and (guess or (table[:, 0] != 1).any()):
        raise ValueError("controlnet_conditioning_scale / control_guidance_start / control_guidance_end / guess_mode need a sampler "
                         "with a ControlNet")
    if not has_features and (table[:, 1] != 1).any():
        raise ValueError("adapter_conditioning_scale / adapter_conditioning_factor need adapter_features")
    if guess and pag_on:
        raise ValueError("guess_mode together with perturbed-attention guidance (pag_scale > 0) is not supported")
    if guess and tiles_on:
        raise ValueError("guess_mode together with tiles is not supported")
    if cache_interval > 1:
        raise ValueError("a conditioning table together with a feature cache (interval > 1) is not supported")
    return table, guess


def _build_consistency(n_steps, timesteps, alphas_cumprod, kind, final_sigmas_type, cache_interval, latents, anchored, ref, factor, weight,
                       interval, filter, noise, table):
    """(table, factor, filter id, ref, noise) of a ``Sampler.run`` - float32 [n_steps, 4], two ints, the reference and the noise slabs (or
    None) as contiguous f32 tensors on the latents' device - or None: no consistency, the call of before.  Everything is checked here,
    before anything is launched."""
    if ref is None:
        given = [k for k, on in (("consistency_factor", factor != 4), ("consistency_weight", weight != 1.0),
                                 ("consistency_interval", interval is not None), ("consistency_filter", filter != "bilinear"),
                                 ("consistency_noise", noise is not None), ("consistency", table is not None)) if on]
        if given:
            raise ValueError(f"{', '.join(given)} need consistency_ref: the reference whose low band the state keeps")
        return None
    if latents.ndim != 4:
        raise ValueError("consistency_ref needs [B,C,h,w] latents")
    N, fid = check_consistency(factor, filter, int(latents.shape[2]), int(latents.shape[3]), cache_interval)
    if not isinstance(ref, torch.Tensor) or tuple(ref.shape) != tuple(latents.shape):
        raise ValueError(f"consistency_ref must be a tensor of the latents' shape {tuple(latents.shape)}, got "
                         f"{tuple(ref.shape) if isinstance(ref, torch.Tensor) else ref!r}")
    if noise is not None and (not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (n_steps,) + tuple(latents.shape)):
        raise ValueError(f"consistency_noise must be a tensor of shape {(n_steps,) + tuple(latents.shape)} (one slab per step of the sampler), "
                         f"got {tuple(noise.shape) if isinstance(noise, torch.Tensor) else noise!r}")
    if table is not None:
        given = [k for k, on in (("consistency_weight", weight != 1.0), ("consistency_interval", interval is not None)) if on]
        if given:
            raise ValueError(f"consistency is an explicit table: it excludes {', '.join(given)}")
        rows = check_consistency_table(table, n_steps)
        if noise is None and (rows[:, 3] != 0).any():
            raise ValueError("consistency: rows with sigma != 0 need consistency_noise")
    else:
        rows = consistency_schedule(timesteps, alphas_cumprod, kind, anchored, weight, FULL_INTERVAL if interval is None else interval,
                                    noisy=noise is not None, final_sigmas_type=final_sigmas_type)
    dev = latents.device
    return (rows, N, fid, ref.to(dev, torch.float32).contiguous(), noise.to(dev, torch.float32).contiguous() if noise is not None else None)


class _Run(NamedTuple):
    """What one ``Sampler.run`` asks of the library: built once every check of ``run`` has passed, consumed by ``Sampler._launch``."""
    entry: str                       # "mrisr_sampler_run" (one context), "mrisr_sampler_run_guided" ([unconditional; conditional],
    contexts: tuple                  # diffusers' order) or "mrisr_sampler_run_pag" ([perturbed; (unconditional;) conditional])
    extra: tuple = ()                # the entry's arguments between the feature count and ``use_graph``
    setters: tuple = ()              # (setter, arguments after the handle): the scalar guidance / PAG values, set before the run
    schedule: Optional[np.ndarray] = None  # the schedule table of this run
    conditioning: Optional[tuple] = None   # (conditioning table, guess)
    skip: bool = False
    consistency: Optional[tuple] = None    # (consistency table, factor, filter id, ref, noise or None): ``_build_consistency``
    tile_plan: Optional[tuple] = None      # ``Sampler._tile_plan``
    cond_at_B: bool = False          # guess mode under classifier-free guidance: the ControlNet sees [B] rows, its image stays [B]


def _pag_run(latents, ehs_c, ehs_u, g, guidance_rescale, s, mask) -> dict:
    """The ``_Run`` fields of a PAG run: the rows [perturbed; conditional] or, with active classifier-free guidance, [perturbed;
    unconditional; conditional]; perturbed rows carry the conditional context."""
    B, phi = latents.shape[0], float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_rescale must lie in [0, 1], got {guidance_rescale!r}")
    # (with PAG the rescale rule needs no active classifier-free guidance: check_guidance sees phi only when CFG can be active)
    cfg_given = ehs_u is not None and float(g) != 1.0
    with_cfg = check_guidance(g, phi if cfg_given else 0.0, ehs_c.shape, None if ehs_u is None else ehs_u.shape, B)
    if latents.ndim != 4 or int(np.prod(latents.shape[1:])) % 4:
        raise ValueError("pag_scale > 0 needs [B,C,h,w] latents with C*h*w a multiple of 4")
    if ehs_c.ndim != 3 or ehs_c.shape[0] not in (1, B):
        raise ValueError(f"encoder_hidden_states must be [1, L, D] or [{B}, L, D], got {tuple(ehs_c.shape)}")
    return dict(entry="mrisr_sampler_run_pag", contexts=(ehs_c, ehs_u, ehs_c) if with_cfg else (ehs_c, ehs_c),
                extra=(1 if with_cfg else 0,),
                setters=(("mrisr_sampler_set_guidance", (float(g), phi)), ("mrisr_sampler_set_pag", (mask, s))))


def _guided_run(latents, ehs_c, ehs_u, g, phi, guess) -> dict:
    """The ``_Run`` fields of a run under classifier-free guidance."""
    if int(np.prod(latents.shape[1:])) % 4:
        raise ValueError("guided sampling needs C*h*w of the latents to be a multiple of 4")
    return dict(entry="mrisr_sampler_run_guided", contexts=(ehs_u, ehs_c), setters=(("mrisr_sampler_set_guidance", (g, phi)),),
                cond_at_B=guess)


class Sampler:
    """Owns a C-ABI sampler (device tables + the captured step graph) for one (unet, controlnet, schedule)."""

    def __init__(self, unet: UNet2DConditionModel, scheduler, controlnet: Optional[ControlNetModel] = None,
                 kind: str = "ddim", clip_sample_range: float = 0.0):
        """``kind``: "ddim" (eta 0), "resshift" (res_srdiff.py:84-96), "ddpm" (ancestral, diffusers DDPMScheduler.step with
        "fixed_small" variance; ``clip_sample_range`` > 0 clips the predicted x0 as diffusers' ``clip_sample`` does), or one of the
        deterministic multistep solvers "unipc" (UniPC bh2) / "dpmsolver++" (DPM-Solver++ 2M), whose options come from the scheduler
        (``UniPCMultistepScheduler`` / ``DPMSolverMultistepScheduler``) or from ``set_solver``.  Given ``lr_latents``, a multistep run
        integrates x - LR: the probability-flow ODE of the reference's shift process, not its stochastic step."""
        kinds = {"ddim": L.STEP_DDIM, "resshift": L.STEP_RESSHIFT, "ddpm": L.STEP_DDPM, "unipc": L.STEP_UNIPC,
                 "dpmsolver++": L.STEP_DPMSOLVERPP}
        if kind not in kinds:
            raise ValueError(f"unknown sampler kind {kind!r}")
        solver = None
        if kind in MULTISTEP_KINDS:
            if clip_sample_range > 0:
                raise ValueError("clip_sample_range belongs to the DDPM step; the multistep solvers do not clip")
            if getattr(scheduler, "kind", kind) != kind:
                raise ValueError(f"a {type(scheduler).__name__} cannot drive Sampler(kind={kind!r})")
            solver = check_solver(kind, getattr(scheduler, "solver_order", 2), getattr(scheduler, "final_sigmas_type", "zero"),
                                  getattr(scheduler, "lower_order_final", True), getattr(scheduler, "disable_corrector", ()))
            if len(scheduler.timesteps) > 1 and not bool((scheduler.timesteps[1:] < scheduler.timesteps[:-1]).all()):
                raise ValueError("multistep solvers need strictly decreasing timesteps")
        self.unet, self.controlnet, self.kind = unet, controlnet, kind
        self.tiles = None  # (t_h, t_w, o_h, o_w, window) once set_tiles turned tiling on
        self.cache_interval, self.cache_depth = 1, 1  # set_cache changes them
        ts = scheduler.timesteps.detach().cpu().to(torch.int64).numpy().copy()
        ac = scheduler.alphas_cumprod.detach().cpu().to(torch.float32).numpy().copy()
        self.n_steps = len(ts)
        self._timesteps, self._n_train = ts, len(ac)  # what ``step_schedule`` needs to build a table for this sampler
        self._alphas_cumprod = ac                     # ... and ``consistency_schedule``
        # what the previous run left in the library: a schedule table, a conditioning table, the skip flag, a consistency table
        self._scheduled, self._conditioned, self._skipping, self._consistent = False, False, False, False
        self._h = C.c_void_p()
        L.check(L.lib().mrisr_sampler_create(unet._h, controlnet._h if controlnet is not None else None,
                                             kinds[kind],
                                             ts.ctypes.data_as(C.c_void_p), int(len(ts)),
                                             ac.ctypes.data_as(C.c_void_p), int(len(ac)), C.byref(self._h)))
        if clip_sample_range > 0:
            L.check(L.lib().mrisr_sampler_set_clip(self._h, float(clip_sample_range)))
        if solver is not None:
            self.set_solver(*solver)

    def __del__(self):
        try:
            if self._h.value:
                L.lib().mrisr_sampler_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def set_solver(self, solver_order: int = 2, final_sigmas_type: str = "zero", disable_corrector=()):
        """Multistep kinds: change the solver options for the next ``run`` (the step graph is captured again when they change).
        A sampler built on a ``UniPCMultistepScheduler`` / ``DPMSolverMultistepScheduler`` starts with that scheduler's options,
        one built on a plain table with order 2 and the "zero" final point."""
        if self.kind not in MULTISTEP_KINDS:
            raise ValueError("solver options belong to the multistep kinds")
        order, final, disable = check_solver(self.kind, solver_order, final_sigmas_type, True, disable_corrector)
        arr = (C.c_int * max(1, len(disable)))(*disable)
        L.check(L.lib().mrisr_sampler_set_solver(self._h, order, 1 if final == "zero" else 0, 1, arr if disable else None, len(disable)))
        self.solver_order, self.final_sigmas_type, self.disable_corrector = order, final, disable

    def set_cache(self, interval: int = 1, depth: int = 1):
        """DeepCache-style feature cache for the next ``run`` (Ma et al. 2023).  With ``interval`` N > 1, step i
        of a run over [first, last) is a full forward when (i - first) % N == 0 and otherwise a shallow one: only the encoder up to
        skip ``depth`` and the decoder stages from the one that consumes it, started from the deep feature the last full step left.
        Fewer launches per step for a bounded deviation from the uncached run.  ``interval=1`` (the default) is no cache at all:
        the step graph and the result of a sampler that never had one.  Changing either value captures the step graphs again."""
        interval, depth = check_cache(interval, depth, int(L.lib().mrisr_model_num_skips(self.unet._h)), self.controlnet is not None)
        self._check_cache_with(interval)
        if self._skipping:  # skip_neutral is an argument of each run: what the last one left in the library is not a conflict
            L.check(L.lib().mrisr_sampler_set_skip(self._h, 0))
            self._skipping = False
        if self._consistent:  # likewise consistency_ref
            L.check(L.lib().mrisr_sampler_set_consistency(self._h, 0, 0, None, 0, None, None))
            self._consistent = False
        L.check(L.lib().mrisr_sampler_set_cache(self._h, interval, depth))
        self.cache_interval, self.cache_depth = interval, depth

    def _check_cache_with(self, interval: int):
        """What a feature cache of ``interval`` excludes on this sampler as it stands: FreeU on the UNet (which carries that state; ``run``
        takes no argument for it) and tiles.  ``set_cache`` asks with the interval it is about to set, ``run`` with the one that is set."""
        if interval > 1 and self.unet.freeu is not None:
            raise ValueError("a feature cache (interval > 1) together with FreeU (unet.enable_freeu) is not supported")
        if interval > 1 and self.tiles is not None:
            raise ValueError("a feature cache (interval > 1) together with tiles is not supported")

    @property
    def divisor(self) -> int:
        """The UNet's divisibility rule for the latents' h and w: 2^(levels-1)."""
        return 2 ** (len(self.unet.config.block_out_channels) - 1)

    def set_tiles(self, tile=None, overlap=0, window: str = "gaussian"):
        """Tiled sampling for the next ``run`` (MultiDiffusion with Mixture-of-Diffusers' Gaussian weights).  The
        latent canvas is cut into tiles of ``tile`` latent pixels (an int or (h, w)) that overlap by ``overlap``; every step runs ONE
        forward on the batch of all tiles (``tile_rows`` tells how many rows that is) and blends the tile predictions with ``window``
        ("gaussian" / "uniform") before the reverse step, which stays on the canvas.  Callers keep passing canvas-shaped arguments.
        ``tile=None`` (the default) turns tiling off: the step graph and the result of a sampler that never had it; so does a tile that
        covers the canvas.  Not together with a feature cache."""
        if tile is None:
            L.check(L.lib().mrisr_sampler_set_tiles(self._h, 0, 0, 0, 0, 0))
            self.tiles = None
            return
        t_h, t_w, o_h, o_w, window = check_tiles(tile, overlap, window, self.divisor, self.cache_interval > 1)
        L.check(L.lib().mrisr_sampler_set_tiles(self._h, t_h, t_w, o_h, o_w, L.TILE_WINDOWS[window]))
        self.tiles = (t_h, t_w, o_h, o_w, window)

    def _tile_plan(self, h: int, w: int):
        """(origins_y, origins_x, t_h, t_w) of a canvas of h x w latents, or None when the run is not tiled (off, or one tile)."""
        if self.tiles is None:
            return None
        t_h, t_w, o_h, o_w, window = self.tiles
        d = self.divisor
        if h <= 0 or w <= 0 or h % d or w % d:
            raise ValueError(f"tiled sampling needs latents whose h and w are multiples of {d}, got {h} x {w}")
        oy, ox = tile_tables(h, t_h, o_h, window)[0], tile_tables(w, t_w, o_w, window)[0]
        return None if len(oy) * len(ox) == 1 else (oy, ox, min(t_h, h), min(t_w, w))

    def tile_rows(self, B: int, h: int, w: int, guided: bool = False) -> int:
        """Rows of the forward a run on [B, C, h, w] latents uses: B (2B when ``guided``) times the number of tiles."""
        plan = self._tile_plan(int(h), int(w))
        return int(B) * (2 if guided else 1) * (len(plan[0]) * len(plan[1]) if plan else 1)

    def _tile_operands(self, plan, h, w, ehs, cond, feats):
        """The timestep-invariant operands of a tiled run, once per run: context rows T times, the condition image cropped per tile at
        8 x origin, every adapter feature (computed ONCE on the whole canvas condition) cropped per tile at origin / its scale."""
        oy, ox, t_h, t_w = plan
        d = self.divisor
        if cond is not None and tuple(cond.shape[-2:]) != (8 * h, 8 * w):
            raise ValueError(f"controlnet_cond must be [B, C, {8 * h}, {8 * w}] for latents of {h} x {w}, got {tuple(cond.shape)}")
        scales = []
        for f in feats:
            r = h // f.shape[2] if f.ndim == 4 and 0 < f.shape[2] <= h else 0
            if r < 1 or r > d or r & (r - 1) or f.shape[2] * r != h or f.shape[3] * r != w:
                raise ValueError(f"adapter features must be [B, C, h / s, w / s] of the {h} x {w} latents with s a power of two <= {d}, "
                                 f"got {tuple(f.shape)}")
            scales.append(r)
        ehs = ehs.repeat_interleave(len(oy) * len(ox), dim=0).contiguous()
        if cond is not None:
            cond = _tile_crops(cond, [8 * y for y in oy], [8 * x for x in ox], 8 * t_h, 8 * t_w)
        feats = [_tile_crops(f, [y // r for y in oy], [x // r for x in ox], t_h // r, t_w // r) for f, r in zip(feats, scales)]
        return ehs, cond, feats

    def set_range(self, first_step: int, last_step: int):
        """Run only steps [first_step, last_step) of the schedule on the next ``run`` (resume / inspection).  The multistep kinds start
        COLD at ``first_step`` (order 1, no corrector: the history of earlier steps is gone), so a split run of theirs is not the
        full run; the first-order kinds reproduce it."""
        L.check(L.lib().mrisr_sampler_set_range(self._h, int(first_step), int(last_step)))

    def run(self, latents: torch.Tensor, encoder_hidden_states: torch.Tensor, lr_latents: Optional[torch.Tensor] = None,
            step_noise: Optional[torch.Tensor] = None, controlnet_cond: Optional[torch.Tensor] = None,
            adapter_features: Optional[Sequence[torch.Tensor]] = None, pag_scale: float = 0.0, pag_applied_layers=("mid",),
            pag_adaptive_scale: float = 0.0, guidance_interval=None, pag_interval=None, freeu_interval=None, schedule=None,
            skip_neutral: bool = False, consistency_ref: Optional[torch.Tensor] = None, consistency_factor: int = 4,
            consistency_weight: float = 1.0, consistency_interval=None, consistency_filter: str = "bilinear",
            consistency_noise: Optional[torch.Tensor] = None, consistency=None,
            controlnet_conditioning_scale: float = 1.0, control_guidance_start: float = 0.0, control_guidance_end: float = 1.0,
            adapter_conditioning_scale: float = 1.0, adapter_conditioning_factor: float = 1.0, guess_mode: bool = False,
            conditioning=None, use_graph: bool = True, guidance_scale: float = 1.0, guidance_rescale: float = 0.0,
            uncond_hidden_states: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Advance ``latents`` [B,C,h,w] (f32, updated IN PLACE) through every timestep.

        Low-frequency consistency (ILVR, Choi et al. 2021): with ``consistency_ref`` [B,C,h,w] - for a
        super-resolver the LR latents - every step ends with ``x <- x + w_i phi_N(y_i - x)``, ``y_i = alpha_i ref + beta_i lr + sigma_i z_i``
        the reference at the noise level of the state the step produced (``consistency_schedule``) and ``phi_N`` the low-pass filter
        "average over N x N blocks, upsample by N" with N = ``consistency_factor`` (2..8, dividing h and w; small: the reference decides
        nearly everything, large: only the coarse anatomy) and ``consistency_filter`` "bilinear" or "nearest" (an exact projection: at
        weight 1 the block means of the state ARE those of ``y_i``).  ``consistency_weight`` w >= 0 applies inside
        ``consistency_interval`` (a ``(start, end)`` pair of fractions of the run, the rule of ``guidance_interval``; ILVR's conditioning
        range) and 0 outside.  ``consistency_noise`` [n_steps,B,C,h,w]: the z_i, which turn the sigma column on (ILVR's noised reference);
        without it the reference is not noised.  ``consistency``: an explicit ``[n_steps, 4]`` table ``{w, alpha, beta, sigma}``
        (``check_consistency_table``) instead of the weight and the interval.  The captured step reads its row from the table, so other
        weights and intervals replay the same graph; another factor, filter, reference buffer or noise buffer captures again.  A
        ``consistency_ref`` (or ``consistency_noise``) that is already on the device, contiguous and float32 is passed by ADDRESS, not
        copied: a caller who refills the same buffer between runs replays the graph.  It acts on the canvas after the step, so it
        composes with every step kind, guidance, PAG, tiles, ``skip_neutral`` (a step of weight 0 still launches the kernel, which returns
        at once), ControlNet, adapter features, FreeU and ``set_range``.  Not with a feature cache.  The canvas must fit the kernel's
        LDS scratch (``check_consistency``).  Consistency is on exactly when ``consistency_ref`` is given; without it the other six are
        refused and the call is the one of before: same launches, same bits, same captures.

        Skipping: with ``skip_neutral=True`` each step runs only the rows and networks its table rows need
        (``step_variants``): a step whose schedule row is neutral (``g == 1`` and ``s == 0``) forwards the B conditional rows alone, a
        step with ControlNet scale 0 launches no ControlNet, a step with adapter scale 0 takes no features.  In exact arithmetic the
        result is the one without the option; in floating point it differs by rounding on the skipped steps.  Each variant is its own
        captured graph, taken the first time a run needs it; ``last_run_stats`` tells what the run did.  Not with a feature cache.  The
        default leaves everything as it is: same launches, same bits, same captures.

        Conditioning strength: ``controlnet_conditioning_scale`` (the ControlNet residuals times this),
        ``control_guidance_start`` / ``control_guidance_end`` (fractions of the run outside which the residuals count 0),
        ``adapter_conditioning_scale`` / ``adapter_conditioning_factor`` (the adapter features times the scale on the first
        ``int(n * factor)`` steps, 0 afterwards) build a conditioning table with ``conditioning_schedule``; ``conditioning``: an explicit
        ``[n_steps, 4]`` table (``check_conditioning``) instead of those five.  The captured step reads the strengths from the table, so
        other values replay the same graph; a step with scale 0 still runs the ControlNet unless ``skip_neutral`` is given.  ``guess_mode`` (diffusers'): residual k is
        weighted by ``guess_mode_weights``; under classifier-free guidance the ControlNet then runs on the conditional rows only and the
        unconditional rows get no residual (``controlnet_cond`` stays [B]).  Not with PAG or tiles.  With none of the seven the call is
        the one without a table: same launches, same bits.  A table is refused together with a feature cache.

        Per-step strengths: ``pag_adaptive_scale`` (the PAG scale decays as ``step_schedule`` states),
        ``guidance_interval`` / ``pag_interval`` / ``freeu_interval`` (``(start, end)`` fractions of the run: outside, that control is
        neutral) build a schedule table with ``step_schedule`` from the scalar arguments - inside an interval these are the values - and
        the UNet's ``enable_freeu`` state; the captured step reads its strengths from the table, so other values replay the same graph.
        Each needs its control to be active (``freeu_interval``: FreeU on the UNet).  ``schedule``: an explicit ``[n_steps, 8]`` table
        (``check_schedule``) instead of those four; the scalar arguments then only choose the kind of run (``pag_scale > 0``: a PAG run;
        ``uncond_hidden_states`` with ``guidance_scale != 1``: the unconditional half) and their values are not read.  Row i belongs to
        step i of the schedule also under ``set_range``.  With none of the five the call is the one without a table: same launches,
        same bits.  A step whose row is neutral still costs a guided step unless ``skip_neutral`` is given.

        FreeU needs no argument: a UNet with ``enable_freeu`` applies it in every step, with every option below
        except the feature cache.

        Perturbed-attention guidance (Ahn et al. 2024): with ``pag_scale`` s > 0 every step also predicts eps_p -
        the same network with the self-attention map of the blocks ``pag_applied_layers`` selects (``check_pag``) replaced by the identity
        - in the same forward (perturbed rows first: 2B rows, 3B with classifier-free guidance) and steps with
        eps = eps_u + g (eps_c - eps_u) + s (eps_c - eps_p) (eps_u := eps_c without CFG), then the ``guidance_rescale`` rule.  No
        unconditional prompt is needed.  ``pag_scale=0`` (the default) is the call without it.  Not with a feature cache.

        Classifier-free guidance: with ``uncond_hidden_states`` ([1,L,D] or [B,L,D]) and ``guidance_scale`` g != 1 every step runs
        ONE forward of 2B rows (unconditional rows first) and the fused guided step: eps = eps_u + g (eps_c - eps_u), then, for
        ``guidance_rescale`` phi > 0, eps *= phi std(eps_c) / std(eps) + (1 - phi) per sample (Lin et al. 2023, sec. 3.4).  Everything
        else is given at [B] as without guidance.  Without these arguments, or at g == 1, the call is the unguided one."""
        if latents.dtype != torch.float32 or not latents.is_contiguous():
            raise ValueError("latents must be contiguous float32 (updated in place)")
        if self.kind in MULTISTEP_KINDS:
            if step_noise is not None:
                raise ValueError(f"kind={self.kind!r} is deterministic: step_noise is refused")
            if latents.ndim != 4 or int(np.prod(latents.shape[1:])) % 4:
                raise ValueError("the multistep solvers need [B,C,h,w] latents with C*h*w a multiple of 4")
            if lr_latents is not None and tuple(lr_latents.shape) != tuple(latents.shape):
                raise ValueError(f"lr_latents must have the latents' shape {tuple(latents.shape)}, got {tuple(lr_latents.shape)}")
        self._check_cache_with(self.cache_interval)
        skip = check_skip(skip_neutral, self.cache_interval)
        plan = None
        if self.tiles is not None:  # a tiled run: the canvas and everything shaped after it is checked here, before any launch
            if latents.ndim != 4:
                raise ValueError("tiled sampling needs [B,C,h,w] latents")
            plan = self._tile_plan(latents.shape[2], latents.shape[3])
        pag_mask = check_pag(pag_scale, pag_applied_layers, transformer_block_names(self.unet.config),
                             self.cache_interval > 1, self.unet.fp8_attention)
        table = _build_schedule(self.n_steps, self._timesteps, self._n_train, self.unet.freeu, schedule, pag_adaptive_scale,
                                guidance_interval, pag_interval, freeu_interval, guidance_scale, guidance_rescale, pag_scale, bool(pag_mask),
                                uncond_hidden_states is not None)
        conditioning = _build_conditioning(self.n_steps, self.controlnet is not None, self.tiles is not None, self.cache_interval,
                                           conditioning, controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                                           adapter_conditioning_scale, adapter_conditioning_factor, guess_mode, bool(pag_mask),
                                           bool(adapter_features))
        cons = _build_consistency(self.n_steps, self._timesteps, self._alphas_cumprod, self.kind, getattr(self, "final_sigmas_type", "zero"),
                                  self.cache_interval, latents, self.kind == "resshift" or lr_latents is not None, consistency_ref,
                                  consistency_factor, consistency_weight, consistency_interval, consistency_filter, consistency_noise,
                                  consistency)
        if pag_mask:
            kind = _pag_run(latents, encoder_hidden_states, uncond_hidden_states, guidance_scale, guidance_rescale, float(pag_scale), pag_mask)
        elif check_guidance(guidance_scale, guidance_rescale, encoder_hidden_states.shape,
                            None if uncond_hidden_states is None else uncond_hidden_states.shape, latents.shape[0]):
            kind = _guided_run(latents, encoder_hidden_states, uncond_hidden_states, float(guidance_scale), float(guidance_rescale),
                               conditioning is not None and conditioning[1])
        else:
            kind = dict(entry="mrisr_sampler_run", contexts=(encoder_hidden_states,))
        return self._launch(_Run(schedule=table, conditioning=conditioning, skip=skip, consistency=cons, tile_plan=plan, **kind), latents, lr_latents,
                            step_noise, controlnet_cond, adapter_features, use_graph)

    def _launch(self, run: _Run, latents, lr_latents, step_noise, controlnet_cond, adapter_features, use_graph):
        """The one path into the library.  Timestep-invariant plumbing, once per run: each of the K contexts at B rows, images and
        features K times, then their tiles.  Then, every Python-side check having passed, what the run sets in the library: the scalar
        setters, the tables of this run (a table an earlier run left there is cleared when this one has none), the skip flag."""
        B, dev, K, plan = latents.shape[0], latents.device, len(run.contexts), run.tile_plan
        feats = list(adapter_features or [])
        if K > 1 or plan is not None:  # (the plain untiled call leaves a wrong batch to the library's own check)
            if controlnet_cond is not None and controlnet_cond.shape[0] != B:
                raise ValueError(f"controlnet_cond must carry the latents' batch {B}, got {tuple(controlnet_cond.shape)}")
            for f in feats:
                if f.shape[0] != B:
                    raise ValueError(f"adapter features must carry the latents' batch {B}, got {tuple(f.shape)}")

        def rows(t):  # [B] -> [K B]
            return (t.to(dev) if K == 1 else torch.cat([t.to(dev)] * K)).contiguous()
        parts = [e.to(dev) if e.shape[0] == B else e.to(dev).expand(B, -1, -1) for e in run.contexts]
        ehs = (parts[0] if K == 1 else torch.cat(parts)).contiguous()
        lr = lr_latents.to(dev, torch.float32).contiguous() if lr_latents is not None else None
        nz = step_noise.to(dev, torch.float32).contiguous() if step_noise is not None else None
        cond = (controlnet_cond.to(dev).contiguous() if run.cond_at_B else rows(controlnet_cond)) if controlnet_cond is not None else None
        feats = [rows(f) for f in feats]
        if plan is not None:  # the K B rows, then their tiles: row (b, ti) of the forward is b * T + ti
            ehs, cond, feats = self._tile_operands(plan, latents.shape[2], latents.shape[3], ehs, cond, feats)
        keep = (ehs, lr, nz, cond, feats)  # kept alive until the stream has consumed them
        t_lat, t_e = L.as_tensor(latents), L.as_tensor(ehs)
        t_lr = L.as_tensor(lr) if lr is not None else None
        # step noise is [n_stochastic_steps, B, C, h, w]: described to the C ABI as a stack of [B,C,h,w] slabs
        t_nz = L.as_tensor(nz, shape=(nz.shape[0] * nz.shape[1],) + tuple(nz.shape[2:])) if nz is not None else None
        t_c = L.as_tensor(cond) if cond is not None else None
        f_arr = L.tensor_array([L.as_tensor(f) for f in feats])
        lib = L.lib()
        for setter, args in run.setters:
            L.check(getattr(lib, setter)(self._h, *args))
        if run.schedule is not None or self._scheduled:
            table = run.schedule
            L.check(lib.mrisr_sampler_set_schedule(self._h, table.ctypes.data_as(C.c_void_p), int(table.shape[0]))
                    if table is not None else lib.mrisr_sampler_set_schedule(self._h, None, 0))
            self._scheduled = table is not None
        if run.conditioning is not None or self._conditioned:
            table, guess = run.conditioning or (None, False)
            L.check(lib.mrisr_sampler_set_conditioning(self._h, table.ctypes.data_as(C.c_void_p), int(table.shape[0]), 1 if guess else 0)
                    if table is not None else lib.mrisr_sampler_set_conditioning(self._h, None, 0, 0))
            self._conditioned = table is not None
        if run.skip or self._skipping:
            L.check(lib.mrisr_sampler_set_skip(self._h, 1 if run.skip else 0))
            self._skipping = run.skip
        if run.consistency is not None:
            rows, N, fid, ref, cnz = run.consistency
            keep += (ref, cnz)
            t_ref = L.as_tensor(ref)
            t_cnz = L.as_tensor(cnz, shape=(cnz.shape[0] * cnz.shape[1],) + tuple(cnz.shape[2:])) if cnz is not None else None
            L.check(lib.mrisr_sampler_set_consistency(self._h, N, fid, rows.ctypes.data_as(C.c_void_p), int(rows.shape[0]), C.byref(t_ref),
                                                      C.byref(t_cnz) if t_cnz else None))
            self._consistent = True
        elif self._consistent:
            L.check(lib.mrisr_sampler_set_consistency(self._h, 0, 0, None, 0, None, None))
            self._consistent = False
        L.check(getattr(lib, run.entry)(self._h, C.byref(t_lat), C.byref(t_lr) if t_lr else None, C.byref(t_nz) if t_nz else None,
                                        C.byref(t_e), C.byref(t_c) if t_c else None, f_arr if feats else None, len(feats), *run.extra,
                                        1 if use_graph else 0, L.stream_ptr()))
        self._keep = keep
        return latents

    @property
    def last_run_stats(self) -> dict:
        """What the last ``run`` did, from the library's own count: ``unet_rows`` (the sum over its steps of the rows of the UNet forward),
        ``controlnet_steps`` (steps that ran the ControlNet), ``feature_steps`` (steps that took adapter features), ``variants`` (distinct
        step variants, ``step_variants``) and ``captures`` (step graphs this sampler has captured so far)."""
        out = (C.c_int64 * 4)()
        L.check(L.lib().mrisr_sampler_run_stats(self._h, out))
        return {"unet_rows": int(out[0]), "controlnet_steps": int(out[1]), "feature_steps": int(out[2]), "variants": int(out[3]),
                "captures": int(L.lib().mrisr_sampler_num_captures(self._h))}

@torch.no_grad()
def log_validation(unet, controlnet, vae, val_dataloader, noise_scheduler, weight_dtype, accelerator, fixed_embeds,
                   num_inference_steps=20, adapter=None, solver=None, cache_interval=1, cache_depth=1, tile=None, tile_overlap=0,
                   tile_window="gaussian", pag_scale=0.0, pag_applied_layers=("mid",), freeu=None, pag_adaptive_scale=0.0,
                   guidance_interval=None, pag_interval=None, freeu_interval=None, skip_neutral=False, consistency_factor=None,
                   consistency_weight=1.0, consistency_interval=None, consistency_filter="bilinear", controlnet_conditioning_scale=1.0,
                   control_guidance_start=0.0, control_guidance_end=1.0, adapter_conditioning_scale=1.0, adapter_conditioning_factor=1.0,
                   guess_mode=False, guidance_scale=1.0, guidance_rescale=0.0, uncond_embeds=None):
    """Drop-in for the reference's validation sampler (res_srdiff.py:35-105): same inputs, same PIL panel out.
    The timestep loop is one fused sampler call; the per-step noise is drawn up front from the same global RNG
    stream, in the same order, as the reference's per-step ``torch.randn_like`` calls.  ``adapter`` (a T2I-Adapter):
    its features of the condition image, at the LR image's own size so that they land on the latents, enter every step.
    ``guidance_scale`` / ``guidance_rescale`` / ``uncond_embeds`` (the empty caption's embedding, [1,L,D]): classifier-free
    guidance as in ``Sampler.run``; the defaults leave the result unchanged.  ``solver`` ("unipc" / "dpmsolver++"): sample the panel
    with that LR-anchored deterministic multistep solver (the scheduler's solver options when it carries any) instead of the
    reference's stochastic step; no step noise is drawn then.  ``None``: the reference's sampler.  ``cache_interval`` /
    ``cache_depth``: the feature cache of ``Sampler.set_cache``; the defaults leave the panel unchanged.  ``tile`` / ``tile_overlap`` /
    ``tile_window``: tiled sampling as in ``Sampler.set_tiles`` (latent pixels); the defaults leave the panel unchanged.
    ``pag_scale`` / ``pag_applied_layers``: perturbed-attention guidance as in ``Sampler.run``; the defaults leave the panel unchanged.
    ``freeu``: a ``(s1, s2, b1, b2)`` tuple turns FreeU on (``unet.enable_freeu``) for this validation run; the UNet's previous FreeU
    state is restored afterwards, also on an error.  ``None``: the UNet's own state is used as it is.
    ``pag_adaptive_scale`` / ``guidance_interval`` / ``pag_interval`` / ``freeu_interval``: the per-step strengths of ``Sampler.run``
    (``step_schedule``); the defaults leave the panel unchanged.
    ``controlnet_conditioning_scale`` / ``control_guidance_start`` / ``control_guidance_end`` / ``adapter_conditioning_scale`` /
    ``adapter_conditioning_factor`` / ``guess_mode``: the conditioning strength of ``Sampler.run`` (``conditioning_schedule``); the
    defaults leave the panel unchanged.
    ``skip_neutral``: as in ``Sampler.run`` - steps leave out the rows and networks the options above make neutral; the default
    leaves the panel unchanged.
    ``consistency_factor`` (an int N in 2..8) turns low-frequency consistency on as in ``Sampler.run``, with the LR anchor latents as the
    reference and ``consistency_weight`` / ``consistency_interval`` / ``consistency_filter`` as there; the reference is not noised (no
    consistency noise is drawn: the global RNG stream is the default one).  ``None``: off, the other three must be at their defaults
    and the panel is unchanged."""
    from PIL import Image

    if consistency_factor is None and (consistency_weight != 1.0 or consistency_interval is not None or consistency_filter != "bilinear"):
        raise ValueError("consistency_weight / consistency_interval / consistency_filter need consistency_factor")

    freeu_vals = None
    if freeu is not None:
        if len(tuple(freeu)) != 4:
            raise ValueError(f"freeu must be a (s1, s2, b1, b2) tuple, got {freeu!r}")
        freeu_vals = check_freeu(*freeu)

    check_skip(skip_neutral, cache_interval)
    if solver is not None:
        check_solver(solver, getattr(noise_scheduler, "solver_order", 2), getattr(noise_scheduler, "final_sigmas_type", "zero"),
                     getattr(noise_scheduler, "lower_order_final", True), getattr(noise_scheduler, "disable_corrector", ()))

    unet.eval()
    if controlnet is not None:
        controlnet.eval()
    dev = accelerator.device
    val_batch = next(iter(val_dataloader))
    hr_raw = val_batch["hr"][0:1].to(dev, dtype=weight_dtype)
    lr_raw = val_batch["lr"][0:1].to(dev, dtype=weight_dtype)
    control_image = prepare_condition_image(lr_raw)
    lr_input = lr_raw.expand(-1, 3, -1, -1) if lr_raw.shape[1] == 1 else lr_raw
    lr_anchor = (vae.encode(lr_input).latent_dist.sample() * vae.config.scaling_factor).to(torch.float32)
    noise_scheduler.set_timesteps(num_inference_steps, device=dev)
    timesteps = noise_scheduler.timesteps
    latents = get_res_shifting_latents(lr_anchor, lr_anchor, timesteps[0], noise_scheduler).contiguous()
    n_noise = sum(1 for i in range(len(timesteps)) if (int(timesteps[i + 1]) if i + 1 < len(timesteps) else 0) > 0)
    if solver is not None:
        n_noise = 0
    step_noise = torch.stack([torch.randn_like(latents) for _ in range(n_noise)]) if n_noise else None
    freeu_prev = unet.freeu
    if freeu_vals is not None:
        unet.enable_freeu(*freeu_vals)
    try:
        sampler = Sampler(unet, noise_scheduler, controlnet, kind=solver if solver is not None else "resshift")
        if cache_interval != 1 or cache_depth != 1:
            sampler.set_cache(cache_interval, cache_depth)
        if tile is not None:
            sampler.set_tiles(tile, tile_overlap, tile_window)
        feats = None
        if adapter is not None:
            cond = control_image if tuple(control_image.shape[-2:]) == tuple(lr_raw.shape[-2:]) else \
                prepare_condition_image(lr_raw, tuple(lr_raw.shape[-2:]))
            feats = adapter(cond.to(torch.float32))
        cons = {} if consistency_factor is None else dict(
            consistency_ref=lr_anchor, consistency_factor=consistency_factor, consistency_weight=consistency_weight,
            consistency_interval=consistency_interval, consistency_filter=consistency_filter)
        sampler.run(latents, fixed_embeds[0:1], lr_latents=lr_anchor, step_noise=step_noise,
                    controlnet_cond=control_image if controlnet is not None else None, adapter_features=feats,
                    guidance_scale=guidance_scale, guidance_rescale=guidance_rescale,
                    uncond_hidden_states=uncond_embeds[0:1] if uncond_embeds is not None else None, pag_scale=pag_scale,
                    pag_applied_layers=pag_applied_layers, pag_adaptive_scale=pag_adaptive_scale, guidance_interval=guidance_interval,
                    pag_interval=pag_interval, freeu_interval=freeu_interval,
                    controlnet_conditioning_scale=controlnet_conditioning_scale, control_guidance_start=control_guidance_start,
                    control_guidance_end=control_guidance_end, adapter_conditioning_scale=adapter_conditioning_scale,
                    adapter_conditioning_factor=adapter_conditioning_factor, guess_mode=guess_mode, skip_neutral=skip_neutral, **cons)
    finally:
        if freeu_vals is not None:
            if freeu_prev is None:
                unet.disable_freeu()
            else:
                unet.enable_freeu(*freeu_prev)
    gen_vis = decode_to_vis(latents.to(weight_dtype), vae)
    hr_vis = decode_to_vis(hr_raw, vae, is_latent=False)
    lr_vis = decode_to_vis(lr_raw, vae, is_latent=False)
    return Image.fromarray(np.hstack([lr_vis, gen_vis, hr_vis]))
