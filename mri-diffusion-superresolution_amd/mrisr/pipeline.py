"""Host-side mirror of the reference's sampler glue (``src/adapters/res_srdiff.py``): same function names, argument
meaning and error behaviour; the arithmetic runs in libmrisr.so.

  get_res_shifting_latents  :7-25      prepare_condition_image :27-33
  log_validation            :35-105    decode_to_vis           :107-122

plus ``sample`` - the timestep loop itself (``:63-96``) as ONE call into the C-ABI sampler, which captures a step
(ControlNet -> UNet -> fused reverse step) into a hipGraph and replays it; no host sync on ``prev_t > 0``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .models import ControlNetModel, UNet2DConditionModel


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
        ts = scheduler.timesteps.detach().cpu().to(torch.int64).numpy().copy()
        ac = scheduler.alphas_cumprod.detach().cpu().to(torch.float32).numpy().copy()
        self.n_steps = len(ts)
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
            if getattr(self, "_h", None) and self._h.value:
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
        L.check(L.lib().mrisr_sampler_set_cache(self._h, interval, depth))
        self.cache_interval, self.cache_depth = interval, depth

    def set_range(self, first_step: int, last_step: int):
        """Run only steps [first_step, last_step) of the schedule on the next ``run`` (resume / inspection).  The multistep kinds start
        COLD at ``first_step`` (order 1, no corrector: the history of earlier steps is gone), so a split run of theirs is not the
        full run; the first-order kinds reproduce it."""
        L.check(L.lib().mrisr_sampler_set_range(self._h, int(first_step), int(last_step)))

    def run(self, latents: torch.Tensor, encoder_hidden_states: torch.Tensor, lr_latents: Optional[torch.Tensor] = None,
            step_noise: Optional[torch.Tensor] = None, controlnet_cond: Optional[torch.Tensor] = None,
            adapter_features: Optional[Sequence[torch.Tensor]] = None, use_graph: bool = True,
            guidance_scale: float = 1.0, guidance_rescale: float = 0.0,
            uncond_hidden_states: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Advance ``latents`` [B,C,h,w] (f32, updated IN PLACE) through every timestep.

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
        if check_guidance(guidance_scale, guidance_rescale, encoder_hidden_states.shape,
                          None if uncond_hidden_states is None else uncond_hidden_states.shape, latents.shape[0]):
            return self._run_guided(latents, encoder_hidden_states, uncond_hidden_states, lr_latents, step_noise, controlnet_cond,
                                    adapter_features, use_graph, float(guidance_scale), float(guidance_rescale))
        dev = latents.device
        ehs = encoder_hidden_states.to(dev).contiguous()
        if ehs.shape[0] != latents.shape[0]:
            ehs = ehs.expand(latents.shape[0], -1, -1).contiguous()
        lr = lr_latents.to(dev, torch.float32).contiguous() if lr_latents is not None else None
        nz = step_noise.to(dev, torch.float32).contiguous() if step_noise is not None else None
        cond = controlnet_cond.to(dev).contiguous() if controlnet_cond is not None else None
        feats = [f.to(dev).contiguous() for f in (adapter_features or [])]
        keep = (ehs, lr, nz, cond, feats)  # noqa: F841  keep alive until the stream has consumed them
        t_lat, t_e = L.as_tensor(latents), L.as_tensor(ehs)
        t_lr = L.as_tensor(lr) if lr is not None else None
        # step noise is [n_stochastic_steps, B, C, h, w]: described to the C ABI as a stack of [B,C,h,w] slabs
        t_nz = L.as_tensor(nz, shape=(nz.shape[0] * nz.shape[1],) + tuple(nz.shape[2:])) if nz is not None else None
        t_c = L.as_tensor(cond) if cond is not None else None
        f_arr = L.tensor_array([L.as_tensor(f) for f in feats])
        L.check(L.lib().mrisr_sampler_run(self._h, C.byref(t_lat), C.byref(t_lr) if t_lr else None,
                                          C.byref(t_nz) if t_nz else None, C.byref(t_e), C.byref(t_c) if t_c else None,
                                          f_arr if feats else None, len(feats), 1 if use_graph else 0, L.stream_ptr()))
        self._keep = keep
        return latents

    def _run_guided(self, latents, ehs_c, ehs_u, lr_latents, step_noise, controlnet_cond, adapter_features, use_graph, g, phi):
        B, dev = latents.shape[0], latents.device
        if int(np.prod(latents.shape[1:])) % 4:
            raise ValueError("guided sampling needs C*h*w of the latents to be a multiple of 4")
        if controlnet_cond is not None and controlnet_cond.shape[0] != B:
            raise ValueError(f"controlnet_cond must carry the latents' batch {B}, got {tuple(controlnet_cond.shape)}")
        for f in (adapter_features or []):
            if f.shape[0] != B:
                raise ValueError(f"adapter features must carry the latents' batch {B}, got {tuple(f.shape)}")
        # timestep-invariant plumbing, once per run: [unconditional rows; conditional rows] (diffusers' order), images and features twice
        ehs2 = torch.cat([e.to(dev).expand(B, -1, -1) for e in (ehs_u, ehs_c)]).contiguous()
        lr = lr_latents.to(dev, torch.float32).contiguous() if lr_latents is not None else None
        nz = step_noise.to(dev, torch.float32).contiguous() if step_noise is not None else None
        cond2 = torch.cat([controlnet_cond.to(dev)] * 2).contiguous() if controlnet_cond is not None else None
        feats2 = [torch.cat([f.to(dev)] * 2).contiguous() for f in (adapter_features or [])]
        keep = (ehs2, lr, nz, cond2, feats2)
        t_lat, t_e = L.as_tensor(latents), L.as_tensor(ehs2)
        t_lr = L.as_tensor(lr) if lr is not None else None
        t_nz = L.as_tensor(nz, shape=(nz.shape[0] * nz.shape[1],) + tuple(nz.shape[2:])) if nz is not None else None
        t_c = L.as_tensor(cond2) if cond2 is not None else None
        f_arr = L.tensor_array([L.as_tensor(f) for f in feats2])
        L.check(L.lib().mrisr_sampler_set_guidance(self._h, g, phi))
        L.check(L.lib().mrisr_sampler_run_guided(self._h, C.byref(t_lat), C.byref(t_lr) if t_lr else None,
                                                 C.byref(t_nz) if t_nz else None, C.byref(t_e), C.byref(t_c) if t_c else None,
                                                 f_arr if feats2 else None, len(feats2), 1 if use_graph else 0, L.stream_ptr()))
        self._keep = keep
        return latents


@torch.no_grad()
def log_validation(unet, controlnet, vae, val_dataloader, noise_scheduler, weight_dtype, accelerator, fixed_embeds,
                   num_inference_steps=20, adapter=None, solver=None, cache_interval=1, cache_depth=1, guidance_scale=1.0,
                   guidance_rescale=0.0, uncond_embeds=None):
    """Drop-in for the reference's validation sampler (res_srdiff.py:35-105): same inputs, same PIL panel out.
    The timestep loop is one fused sampler call; the per-step noise is drawn up front from the same global RNG
    stream, in the same order, as the reference's per-step ``torch.randn_like`` calls.  ``adapter`` (a T2I-Adapter):
    its features of the condition image, at the LR image's own size so that they land on the latents, enter every step.
    ``guidance_scale`` / ``guidance_rescale`` / ``uncond_embeds`` (the empty caption's embedding, [1,L,D]): classifier-free
    guidance as in ``Sampler.run``; the defaults leave the result unchanged.  ``solver`` ("unipc" / "dpmsolver++"): sample the panel
    with that LR-anchored deterministic multistep solver (the scheduler's solver options when it carries any) instead of the
    reference's stochastic step; no step noise is drawn then.  ``None``: the reference's sampler.  ``cache_interval`` /
    ``cache_depth``: the feature cache of ``Sampler.set_cache``; the defaults leave the panel unchanged."""
    from PIL import Image

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
    sampler = Sampler(unet, noise_scheduler, controlnet, kind=solver if solver is not None else "resshift")
    if cache_interval != 1 or cache_depth != 1:
        sampler.set_cache(cache_interval, cache_depth)
    feats = None
    if adapter is not None:
        cond = control_image if tuple(control_image.shape[-2:]) == tuple(lr_raw.shape[-2:]) else \
            prepare_condition_image(lr_raw, tuple(lr_raw.shape[-2:]))
        feats = adapter(cond.to(torch.float32))
    sampler.run(latents, fixed_embeds[0:1], lr_latents=lr_anchor, step_noise=step_noise,
                controlnet_cond=control_image if controlnet is not None else None, adapter_features=feats,
                guidance_scale=guidance_scale, guidance_rescale=guidance_rescale,
                uncond_hidden_states=uncond_embeds[0:1] if uncond_embeds is not None else None)
    gen_vis = decode_to_vis(latents.to(weight_dtype), vae)
    hr_vis = decode_to_vis(hr_raw, vae, is_latent=False)
    lr_vis = decode_to_vis(lr_raw, vae, is_latent=False)
    return Image.fromarray(np.hstack([lr_vis, gen_vis, hr_vis]))
