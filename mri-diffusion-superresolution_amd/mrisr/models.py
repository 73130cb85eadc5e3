"""Host-side mirror of the model objects the reference passes around (duck-typed):

* ``UNet2DConditionModel``  - call surface of diffusers' class as used at reference
  ``src/adapters/res_srdiff.py:73-78``:  ``unet(latents, t, encoder_hidden_states=..., down_block_additional_residuals=...,
  mid_block_additional_residual=...).sample``  (+ ``down_intrablock_additional_residuals`` for T2I-Adapter features).
* ``ControlNetModel``       - ``controlnet(latents, t, encoder_hidden_states=..., controlnet_cond=..., return_dict=False)``
  -> ``(down_res, mid_res)``  (``res_srdiff.py:65-70``).
* ``Adapter_XL``            - the reference's own T2I-Adapter (``src/adapters/modules.py:114-157``), ``sk=True`` semantics.

All arithmetic runs in libmrisr.so (HIP, gfx950); these classes only hold parameters (diffusers / peft / reference
state-dict key names) and marshal device pointers.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L


@dataclass
class UNetConfig:
    """diffusers config keys the path depends on (SD-1.5 defaults)."""
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    down_block_types: Tuple[str, ...] = ("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D",
                                         "DownBlock2D")
    layers_per_block: int = 2
    attention_head_dim: int = 8  # number of heads (diffusers naming quirk)
    cross_attention_dim: int = 768
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    conditioning_channels: int = 3
    conditioning_embedding_out_channels: Tuple[int, ...] = (16, 32, 96, 256)

    @classmethod
    def from_oracle_like(cls, cfg) -> "UNetConfig":
        """Build from any object with the oracle's/diffusers' field names (attn_levels or down_block_types)."""
        if hasattr(cfg, "attn_levels"):
            types = tuple("CrossAttnDownBlock2D" if a else "DownBlock2D" for a in cfg.attn_levels)
        else:
            types = tuple(cfg.down_block_types)
        heads = getattr(cfg, "num_heads", None) or getattr(cfg, "attention_head_dim")
        return cls(in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                   block_out_channels=tuple(cfg.block_out_channels), down_block_types=types,
                   layers_per_block=cfg.layers_per_block, attention_head_dim=heads,
                   cross_attention_dim=cfg.cross_attention_dim, norm_num_groups=cfg.norm_num_groups,
                   norm_eps=cfg.norm_eps,
                   conditioning_channels=getattr(cfg, "cond_channels", 3),
                   conditioning_embedding_out_channels=tuple(getattr(cfg, "cond_embed_channels", (16, 32, 96, 256))))


def transformer_block_names(cfg) -> List[str]:
    """The transformer blocks of a UNet of config ``cfg`` (a ``UNetConfig`` or anything ``UNetConfig.from_oracle_like`` reads), in
    forward order: ``down_blocks.i.attentions.j``, ``mid_block.attentions.0``, ``up_blocks.i.attentions.j`` - 16 for SD-1.5.  Pure
    Python, no device."""
    cfg = cfg if isinstance(cfg, UNetConfig) else UNetConfig.from_oracle_like(cfg)
    attn = [t.startswith("CrossAttn") for t in cfg.down_block_types]
    n = len(attn)
    names = [f"down_blocks.{i}.attentions.{j}" for i in range(n) if attn[i] for j in range(cfg.layers_per_block)]
    names.append("mid_block.attentions.0")
    names += [f"up_blocks.{i}.attentions.{j}" for i in range(n) if attn[n - 1 - i] for j in range(cfg.layers_per_block + 1)]
    return names


def check_freeu(s1, s2, b1, b2) -> Tuple[float, float, float, float]:
    """The argument rules of FreeU (``UNet2DConditionModel.enable_freeu``) on numbers alone (no device is touched):
    each of ``s1``, ``s2``, ``b1``, ``b2`` must be a finite number >= 0.  Returns them as floats in that order; raises ``ValueError``
    naming the bad argument."""
    out = []
    for name, v in (("s1", s1), ("s2", s2), ("b1", b1), ("b2", b2)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"freeu: {name} must be a number >= 0, got {v!r}") from None
        if isinstance(v, bool) or not math.isfinite(f) or f < 0.0:
            raise ValueError(f"freeu: {name} must be finite and >= 0, got {v!r}")
        out.append(f)
    return tuple(out)


def freeu_stage_names(cfg) -> List[str]:
    """The resnets whose inputs FreeU rebalances in a UNet of config ``cfg`` (a ``UNetConfig`` or anything
    ``UNetConfig.from_oracle_like`` reads), in forward order: ``up_blocks.k.resnets.j`` for k in {0, 1} (diffusers' ``resolution_idx``
    rule; stage k = up block k takes (b1, s1) for k = 0 and (b2, s2) for k = 1) and j < layers_per_block + 1.  An up block the UNet
    does not have is skipped.  Pure Python, no device."""
    cfg = cfg if isinstance(cfg, UNetConfig) else UNetConfig.from_oracle_like(cfg)
    n = len(cfg.down_block_types)
    return [f"up_blocks.{k}.resnets.{j}" for k in range(min(2, n)) for j in range(cfg.layers_per_block + 1)]


class _Output:
    def __init__(self, sample):
        self.sample = sample


class _ControlNetOutput:
    def __init__(self, down, mid):
        self.down_block_res_samples = down
        self.mid_block_res_sample = mid


LORA_RANKS_LOW = (4, 8, 12, 16)
LORA_RANKS_HIGH = (32, 48, 64, 80, 96, 112, 128)


def check_lora_rank(rank, conv: bool = False) -> int:
    """The ranks an un-merged adapter may have: 4, 8, 12, 16 everywhere; on the linear targets (``to_q`` / ``to_k`` / ``to_v`` / ``to_out.0``,
    ``ff.net.0.proj``, ``ff.net.2``) also the multiples of 16 from 32 to 128.  ``conv=True``: an adapter on a resnet 3x3
    conv, which stays at 16 or below.  Pure Python, no device; returns the rank, raises ``ValueError`` otherwise."""
    ok = LORA_RANKS_LOW if conv else LORA_RANKS_LOW + LORA_RANKS_HIGH
    if isinstance(rank, bool) or not isinstance(rank, int) or rank not in ok:
        what = "conv LoRA rank (resnet 3x3 adapters stay at 16 or below)" if conv else "LoRA rank"
        raise ValueError(f"{what} {rank!r} is not supported: accepted are 4, 8, 12, 16" + ("" if conv else " and the multiples of 16 from 32 to 128 "
                         "(32, 48, 64, 80, 96, 112, 128)"))
    return rank


def lora_scaling(rank, alpha, use_rslora: bool = False) -> float:
    """The factor ``s`` of ``y = x W^T + s (x A^T) B^T``: ``lora_alpha / r`` (peft's default) or, ``use_rslora``, ``lora_alpha / sqrt(r)``
    (rank-stabilised LoRA).  1.0 without a rank or without an alpha.  Pure Python, no device."""
    if not rank or alpha is None:
        return 1.0
    return float(alpha) / (math.sqrt(rank) if use_rslora else rank)


DORA_KEY = ".lora_magnitude_vector.default.weight"  # in memory, after the module name (peft >= 0.10; older: without ".weight")
DORA_LINEAR_TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2", "proj_in", "proj_out")


def check_dora(sd, use_dora: bool, is_controlnet: bool = False, fp8=False, fp8_attention: bool = False, fp8_train: bool = False) -> None:
    """What a DoRA handle (``use_dora=True``) accepts, checked on the state dict alone: pure Python, no device; raises
    ``ValueError``.  ``sd`` in any accepted key spelling (``lora_keys_from_disk`` normalises it); values need only a ``shape``.

    * ``use_dora`` with ``fp8`` / ``fp8_attention`` / ``fp8_train``, or on a ControlNet handle: refused;
    * a magnitude key without ``use_dora``: refused (the message names ``use_dora=True``);
    * every module with ``lora_A`` / ``lora_B`` is a linear target and carries a magnitude of shape ``[out_features]``, and every
      magnitude has its ``lora_A`` / ``lora_B``; a conv adapter (``conv1`` / ``conv2``) is refused."""
    from .train import lora_keys_from_disk
    sd = lora_keys_from_disk(dict(sd or {}))
    mags = {k[: -len(DORA_KEY)]: v for k, v in sd.items() if k.endswith(DORA_KEY)}
    if not use_dora:
        if mags:
            raise ValueError(f"{next(iter(mags))}: the state dict carries DoRA magnitudes (lora_magnitude_vector); build the model with use_dora=True")
        return
    for flag, on in (("fp8", fp8), ("fp8_attention", fp8_attention), ("fp8_train", fp8_train)):
        if on:
            raise ValueError(f"use_dora=True cannot be combined with {flag}: the fp8 weight copies do not carry the magnitude")
    if is_controlnet:
        raise ValueError("use_dora=True is not supported on a ControlNetModel: DoRA covers the UNet's linear targets")
    mods = {}
    for k, v in sd.items():
        for ab in ("lora_A", "lora_B"):
            if k.endswith(f".{ab}.default.weight"):
                mods.setdefault(k[: -len(f".{ab}.default.weight")], {})[ab] = v
    for m, ab in mods.items():
        a, b = ab.get("lora_A"), ab.get("lora_B")
        if m.endswith(("conv1", "conv2")) or (hasattr(a, "shape") and len(a.shape) == 4 and tuple(a.shape[2:]) != (1, 1)):
            raise ValueError(f"{m}: a conv adapter in a use_dora=True state dict; DoRA covers the linear targets only")
        if not m.endswith(DORA_LINEAR_TARGETS):
            raise ValueError(f"{m}: not a DoRA target; accepted are {', '.join(DORA_LINEAR_TARGETS)}")
        if m not in mags:
            raise ValueError(f"{m}: lora_A / lora_B without {m}{DORA_KEY} in a use_dora=True state dict")
    for m, v in mags.items():
        ab = mods.get(m, {})
        if "lora_A" not in ab or "lora_B" not in ab:
            raise ValueError(f"{m}: a DoRA magnitude without its lora_A / lora_B")
        n = int(ab["lora_B"].shape[0]) if hasattr(ab["lora_B"], "shape") else None
        if hasattr(v, "shape") and (len(v.shape) != 1 or (n is not None and int(v.shape[0]) != n)):
            raise ValueError(f"{m}: the DoRA magnitude must have shape [{n}] (one per output row), got {tuple(v.shape)}")


def dora_magnitude_init(params, lora_state_dict, scale: float) -> Dict[str, torch.Tensor]:
    """peft's DoRA initialisation, ``m = ||W + s B A||`` per output row, for every linear adapter of ``lora_state_dict``: f32 from f32 inputs,
    rows in PyTorch's order (``ff.net.0.proj``: value half, then gate half).  Pure torch, runs on the CPU.  With these magnitudes the scale
    ``m / ||W + s B A||`` is 1 and the DoRA model is the LoRA model of the same ``A`` / ``B``."""
    from .train import lora_keys_from_disk
    lora = lora_keys_from_disk(dict(lora_state_dict))
    out = {}
    for ka, a in lora.items():
        if not ka.endswith(".lora_A.default.weight"):
            continue
        m = ka[: -len(".lora_A.default.weight")]
        b = lora[m + ".lora_B.default.weight"]
        w = params[m + ".weight"] if m + ".weight" in params else params[m + ".base_layer.weight"]
        if a.ndim == 4 and tuple(a.shape[2:]) != (1, 1):
            raise ValueError(f"{m}: DoRA covers the linear targets only, not conv adapters")
        w2 = w.detach().to(torch.float32).reshape(w.shape[0], -1)
        ba = b.detach().to(torch.float32).reshape(w.shape[0], -1) @ a.detach().to(torch.float32).reshape(a.shape[0], -1)
        out[m + DORA_KEY] = torch.linalg.vector_norm(w2 + float(scale) * ba, dim=1)
    return out


def _c_cfg(cfg: UNetConfig, compute_dtype, lora_rank, lora_fused, flash, fp8=False, fp8_attention=False, fp8_train=False) -> L.UNetCfg:
    c = L.UNetCfg()
    c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
    c.num_levels = len(cfg.block_out_channels)
    for i, ch in enumerate(cfg.block_out_channels):
        c.block_out_channels[i] = ch
        c.attn_levels[i] = 1 if cfg.down_block_types[i].startswith("CrossAttn") else 0
    c.layers_per_block = cfg.layers_per_block
    c.num_heads = cfg.attention_head_dim
    c.cross_attention_dim = cfg.cross_attention_dim
    c.norm_num_groups = cfg.norm_num_groups
    c.norm_eps = cfg.norm_eps
    c.cond_channels = cfg.conditioning_channels
    for i, ch in enumerate(cfg.conditioning_embedding_out_channels):
        c.cond_embed_channels[i] = ch
    c.compute_dtype = L.dtype_id(compute_dtype)
    c.lora_rank = lora_rank
    c.lora_fused = 1 if lora_fused else 0
    c.flash_attention = 1 if flash else 0
    c.fp8_linears = 2 if fp8 == "all" else (1 if fp8 else 0)  # True: the K = 320 projections; "all": K = 320 and 640
    c.fp8_attention = 1 if fp8_attention else 0
    c.fp8_train = 1 if fp8_train else 0
    return c


def _check_rows(rows, batch: int, has_context: bool):
    """The ``rows=(lo, hi)`` argument of a window forward, on numbers alone: None, or two ints with ``0 <= lo < hi`` and ``hi - lo`` the
    sample's batch; the context arguments must be absent.  Whether the window lies inside the planned batch is the library's check."""
    if rows is None:
        return None
    try:
        lo, hi = rows
    except (TypeError, ValueError):
        raise ValueError(f"rows must be a (lo, hi) pair of ints, got {rows!r}") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"rows must be a (lo, hi) pair of ints, got {rows!r}")
    if not 0 <= lo < hi or hi - lo != batch:
        raise ValueError(f"rows=(lo, hi) must satisfy 0 <= lo < hi with hi - lo the sample's batch {batch}, got {rows!r}")
    if has_context:
        raise ValueError("rows=(lo, hi): the context is the one cached for the full batch; encoder_hidden_states (and controlnet_cond) must be None")
    return int(lo), int(hi)


class _DeviceModel:
    """Shared plumbing: handle lifetime, state-dict <-> C ABI, timestep marshalling."""
    _create = None

    def __init__(self, config=None, compute_dtype="bf16", lora_rank: int = 0, lora_alpha: Optional[float] = None,
                 lora_fused: bool = True, flash_attention: bool = True, device="cuda", fp8=False, fp8_attention: bool = False,
                 fp8_train: bool = False, use_dora: bool = False, use_rslora: bool = False):
        """``fp8`` / ``fp8_attention`` / ``fp8_train``: BASELINE configs[4] - OCP e4m3 operands on the fp8 MFMA for the K = 320 (``"all"``:
        and 640) projections incl. the LoRA targets, for Q K^T / P V of every attention, and for the FORWARD of the training step
        (backward in bf16, straight through).  Modes of the bf16 engine; off by default.

        ``use_rslora``: the LoRA scale is ``lora_alpha / sqrt(r)`` (``lora_scaling``).  ``use_dora``: the adapters are DoRA adapters - every
        adapted linear carries a magnitude vector (``check_dora``).  Merged (``lora_fused=False``) is the form for
        inference; un-merged the model also trains: ``LoRATrainer`` / ``fit`` then carry the magnitudes as 1-D trainable tensors after all
        ``lora_A`` / ``lora_B``."""
        self.use_dora, self.use_rslora = bool(use_dora), bool(use_rslora)
        check_dora({}, self.use_dora, self._create == "mrisr_controlnet_create", fp8, fp8_attention, fp8_train)  # before any device work
        if lora_rank:  # before anything touches the device: a rank no kernel takes is refused here, not at the first forward
            check_lora_rank(lora_rank)
            if lora_rank > LORA_RANKS_LOW[-1] and lora_fused:
                for flag, on in (("fp8", fp8), ("fp8_attention", fp8_attention), ("fp8_train", fp8_train)):
                    if on:
                        raise ValueError(f"lora_rank={lora_rank} cannot be combined with {flag}: the fp8 LoRA rows are a 16-row buffer")
        if not torch.cuda.is_available():
            raise L.MrisrError("mrisr needs an AMD GPU (gfx950); there is no CPU fallback")
        cfg = config if isinstance(config, UNetConfig) else (UNetConfig() if config is None else UNetConfig.from_oracle_like(config))
        self.config = cfg
        self.device = torch.device(device)
        self.compute_dtype = L.torch_dtype(L.dtype_id(compute_dtype))
        self.lora_rank = lora_rank
        self.lora_scale = lora_scaling(lora_rank, lora_alpha, use_rslora)
        self._params: Dict[str, torch.Tensor] = {}
        self._h = C.c_void_p()
        if (fp8 or fp8_attention or fp8_train) and L.dtype_id(compute_dtype) != L.MRISR_BF16:
            raise ValueError("fp8 projections / attention are modes of the bf16 engine")
        if fp8_attention and not flash_attention:
            raise ValueError("fp8 attention is a mode of the flash kernel")
        if fp8_train and not (fp8 or fp8_attention):
            raise ValueError("fp8_train selects the fp8 forward for training: enable fp8 and / or fp8_attention too")
        self.fp8, self.fp8_attention, self.fp8_train = bool(fp8), bool(fp8_attention), bool(fp8_train)
        self._ccfg = _c_cfg(cfg, compute_dtype, lora_rank, lora_fused, flash_attention, fp8, fp8_attention, fp8_train)
        L.check(getattr(L.lib(), self._create)(C.byref(self._ccfg), C.byref(self._h)))
        self._finalized = False
        self.training = False

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                L.lib().mrisr_model_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ---- nn.Module-like surface ----
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def to(self, *args, **kwargs):
        return self

    def requires_grad_(self, flag: bool = True):
        return self

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = dict(self._params)
        tr = getattr(self, "_trainer", None)
        tr = tr() if tr is not None else None
        if tr is not None:  # a LoRATrainer owns the adapters now: report their trained values, not the loaded ones
            for k, v in tr.state_dict().items():
                sd[k] = v.to(sd[k].dtype) if k in sd else v
        return sd

    def parameters(self):
        return iter(self._params.values())

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """diffusers key names; peft LoRA keys ``<module>.lora_{A,B}.default.weight``."""
        fn = L.lib().mrisr_model_set_param
        self._check_adapter_ranks(sd)  # before any GPU work
        check_dora(sd, self.use_dora, self._create == "mrisr_controlnet_create", self.fp8, self.fp8_attention, self.fp8_train)
        for k, v in sd.items():
            # LoRA keys in any of peft's / diffusers' on-disk forms are accepted (adapter name stripped, "base_model.model." or
            # "unet." prefix); everything else must be a diffusers UNet key as is
            if ".lora_A." in k or ".lora_B." in k or ".lora_magnitude_vector" in k:
                from .train import lora_keys_from_disk
                k = next(iter(lora_keys_from_disk({k: None})))
            self._params[k] = v
            L.push_param(fn, self._h, k, v)
        L.check(L.lib().mrisr_model_set_lora_scale(self._h, C.c_float(self.lora_scale)))
        if self.use_dora:
            L.check(L.lib().mrisr_model_set_dora(self._h, 1))
        L.check(L.lib().mrisr_model_finalize(self._h, L.stream_ptr()))  # raises on missing keys
        self._finalized = True
        return self

    def _check_adapter_ranks(self, sd) -> None:
        """Ranks of the adapters in ``sd``, read from the shapes of their ``lora_A`` tensors ([r, k] on a linear, [r, cin, 3, 3] on a conv)."""
        for k, v in sd.items():
            if ".lora_A." not in k or not hasattr(v, "shape"):
                continue
            r = int(v.shape[0])
            check_lora_rank(r, conv=len(v.shape) == 4)
            if r > LORA_RANKS_LOW[-1] and self._ccfg.lora_fused and self.lora_rank != r:
                raise ValueError(f"{k}: adapter of rank {r} loaded into a model built with lora_rank={self.lora_rank}, lora_fused=True; "
                                 f"build the model with lora_rank={r}")

    @property
    def num_parameters(self) -> int:
        return int(L.lib().mrisr_model_num_params(self._h))

    @property
    def workspace_bytes(self) -> int:
        return int(L.lib().mrisr_model_workspace_bytes(self._h))

    def _timestep(self, t, batch: int) -> torch.Tensor:
        if not torch.is_tensor(t):
            t = torch.tensor(int(t), dtype=torch.int64)
        t = t.to(device=self.device, dtype=torch.int64)
        if t.ndim > 1 or (t.ndim == 1 and t.shape[0] not in (1, batch)):
            raise ValueError(f"timestep must be 0-dim or [B]; got {tuple(t.shape)}")
        return t.contiguous()

    def _skip_shapes(self, B: int, h: int, w: int) -> List[Tuple[int, int, int, int]]:
        n = L.lib().mrisr_model_num_skips(self._h)
        out = []
        for k in range(n + 1):
            s = (C.c_int64 * 4)()
            L.check(L.lib().mrisr_model_skip_shape(self._h, k, B, h, w, s))
            out.append(tuple(int(x) for x in s))
        return out


class UNet2DConditionModel(_DeviceModel):
    _create = "mrisr_unet_create"

    def __call__(self, sample: torch.Tensor, timestep, encoder_hidden_states: Optional[torch.Tensor] = None,
                 down_block_additional_residuals: Optional[Sequence[torch.Tensor]] = None,
                 mid_block_additional_residual: Optional[torch.Tensor] = None,
                 down_intrablock_additional_residuals: Optional[Sequence[torch.Tensor]] = None,
                 return_dict: bool = True, rows: Optional[Tuple[int, int]] = None, **_unused):
        """``rows=(lo, hi)``: a forward on the row window [lo, hi) of the batch the workspace is planned for (by an earlier forward or
        ``set_context``).  ``sample`` and every residual and feature carry the window's ``hi - lo`` rows,
        ``encoder_hidden_states`` must be None - the context is the one cached for the full batch, read at the window's rows - and nothing
        is planned again: a full-batch forward afterwards finds its workspace as it left it."""
        if not self._finalized:
            raise L.MrisrError("load_state_dict() first")
        if sample.ndim != 4 or sample.shape[1] != self.config.in_channels:
            raise ValueError(f"sample must be [B,{self.config.in_channels},h,w]; got {tuple(sample.shape)}")
        sample = sample.to(self.device).contiguous()
        B = sample.shape[0]
        rows = _check_rows(rows, B, encoder_hidden_states is not None)
        t = self._timestep(timestep, B)
        ehs = encoder_hidden_states.to(self.device).contiguous() if encoder_hidden_states is not None else None
        down = [r.to(self.device).contiguous() for r in (down_block_additional_residuals or [])]
        intra = [r.to(self.device).contiguous() for r in (down_intrablock_additional_residuals or [])]
        mid = mid_block_additional_residual.to(self.device).contiguous() if mid_block_additional_residual is not None else None
        out = torch.empty((B, self.config.out_channels, sample.shape[2], sample.shape[3]), dtype=sample.dtype,
                          device=self.device)
        d_arr = L.tensor_array([L.as_tensor(r) for r in down])
        i_arr = L.tensor_array([L.as_tensor(r) for r in intra])
        t_s, t_t, t_o = L.as_tensor(sample), L.as_tensor(t), L.as_tensor(out)
        t_e = L.as_tensor(ehs) if ehs is not None else None
        t_m = L.as_tensor(mid) if mid is not None else None
        if rows is not None:
            L.check(L.lib().mrisr_model_forward_rows(self._h, rows[0], rows[1], C.byref(t_s), C.byref(t_t), d_arr if down else None, len(down),
                                                     C.byref(t_m) if t_m else None, i_arr if intra else None, len(intra), C.byref(t_o),
                                                     L.stream_ptr()))
            return _Output(out) if return_dict else (out,)
        L.check(L.lib().mrisr_unet_forward(self._h, C.byref(t_s), C.byref(t_t), C.byref(t_e) if t_e else None,
                                           d_arr if down else None, len(down), C.byref(t_m) if t_m else None,
                                           i_arr if intra else None, len(intra), C.byref(t_o), L.stream_ptr()))
        return _Output(out) if return_dict else (out,)

    def transformer_block_names(self) -> List[str]:
        """The UNet's transformer blocks in forward order (``transformer_block_names``): entry i is bit i of a PAG block mask."""
        names = transformer_block_names(self.config)
        if len(names) != int(L.lib().mrisr_model_num_transformer_blocks(self._h)):
            raise L.MrisrError("transformer block count differs between the Python config and the device model")
        return names

    def set_pag(self, block_mask: int = 0, first_sample: int = 0, n_samples: int = 0):
        """Perturbed-attention state of this handle (``mrisr_model_set_pag``): until cleared, every forward
        replaces ``attn1`` of samples [first_sample, first_sample + n_samples) in the blocks of ``block_mask`` by
        ``to_out.0(to_v(norm1(h)))``.  No arguments: cleared.  ``Sampler.run(pag_scale=...)`` manages it by itself."""
        L.check(L.lib().mrisr_model_set_pag(self._h, int(block_mask), int(first_sample), int(n_samples)))

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (Si et al. 2023; diffusers' ``enable_freeu``, same names and order): until ``disable_freeu``, every
        forward and every sampler step on this UNet scales, in the resnets of ``freeu_stage_names`` and before hidden and skip are
        concatenated, the first half of the hidden channels by ``b1`` (up block 0) / ``b2`` (up block 1) and the lowest spatial
        frequencies of the skip tensor by ``s1`` / ``s2`` (diffusers' ``fourier_filter``, threshold 1).  The diffusers docs suggest
        ``(0.9, 0.2, 1.5, 1.6)`` for SD-1.5.  Not with the feature cache, not in a training step."""
        vals = check_freeu(s1, s2, b1, b2)  # before the library is touched
        L.check(L.lib().mrisr_model_set_freeu(self._h, 1, *[C.c_float(v) for v in vals]))
        self._freeu = vals

    def disable_freeu(self):
        """Turns FreeU off: the forward is the one of before, bit for bit, with the same launches and workspace."""
        L.check(L.lib().mrisr_model_set_freeu(self._h, 0, C.c_float(1.0), C.c_float(1.0), C.c_float(1.0), C.c_float(1.0)))
        self._freeu = None

    @property
    def freeu(self) -> Optional[Tuple[float, float, float, float]]:
        """``(s1, s2, b1, b2)`` while FreeU is on, else ``None``."""
        return getattr(self, "_freeu", None)

    def cache_shape(self, depth: int, B: int, h: int, w: int) -> Tuple[int, int, int, int]:
        """Logical (B, C, H, W) of the feature cache at ``depth`` for h x w latents: the input of the decoder stage that consumes
        skip ``depth``.  ``forward_cached`` wants it as a [B, H, W, C] tensor of the compute dtype."""
        s = (C.c_int64 * 4)()
        L.check(L.lib().mrisr_unet_cache_shape(self._h, int(depth), int(B), int(h), int(w), s))
        return tuple(int(x) for x in s)

    def forward_cached(self, sample: torch.Tensor, timestep, encoder_hidden_states: Optional[torch.Tensor], cache: torch.Tensor,
                       depth: int, shallow: bool, down_intrablock_additional_residuals: Optional[Sequence[torch.Tensor]] = None):
        """One forward with a DeepCache-style feature cache.  ``cache``: contiguous [B, H, W, C] (NHWC) tensor of the compute dtype
        with (B, C, H, W) = ``cache_shape(depth, ...)``.  ``shallow=False``: the ordinary forward, which also writes ``cache``;
        ``shallow=True``: only the encoder up to skip ``depth`` and the decoder from the stage that consumes it, started from
        ``cache``.  Returns the prediction (a tensor, not an output object)."""
        if not self._finalized:
            raise L.MrisrError("load_state_dict() first")
        if sample.ndim != 4 or sample.shape[1] != self.config.in_channels:
            raise ValueError(f"sample must be [B,{self.config.in_channels},h,w]; got {tuple(sample.shape)}")
        sample = sample.to(self.device).contiguous()
        B, _, h, w = sample.shape
        cb, cc, ch, cw = self.cache_shape(depth, B, h, w)
        if not torch.is_tensor(cache) or not cache.is_cuda or not cache.is_contiguous():
            raise ValueError("cache must be a contiguous tensor on the GPU (NHWC)")
        if cache.dtype != self.compute_dtype:
            raise ValueError(f"cache must be in the compute dtype {self.compute_dtype}, got {cache.dtype}")
        if tuple(cache.shape) != (cb, ch, cw, cc):
            raise ValueError(f"cache must be [B, H, W, C] = {(cb, ch, cw, cc)} for depth {depth}, got {tuple(cache.shape)}")
        t = self._timestep(timestep, B)
        ehs = encoder_hidden_states.to(self.device).contiguous() if encoder_hidden_states is not None else None
        intra = [r.to(self.device).contiguous() for r in (down_intrablock_additional_residuals or [])]
        out = torch.empty((B, self.config.out_channels, h, w), dtype=sample.dtype, device=self.device)
        i_arr = L.tensor_array([L.as_tensor(r) for r in intra])
        t_s, t_t, t_o = L.as_tensor(sample), L.as_tensor(t), L.as_tensor(out)
        t_e = L.as_tensor(ehs) if ehs is not None else None
        t_c = L.as_tensor(cache, layout=L.MRISR_NHWC, shape=(cb, cc, ch, cw))
        L.check(L.lib().mrisr_unet_forward_cached(self._h, C.byref(t_s), C.byref(t_t), C.byref(t_e) if t_e else None,
                                                  i_arr if intra else None, len(intra), int(depth), 1 if shallow else 0,
                                                  C.byref(t_c), C.byref(t_o), L.stream_ptr()))
        return out

    def set_context(self, encoder_hidden_states: torch.Tensor, latent_hw: Tuple[int, int]):
        """Pre-compute the cross-attention K/V of a fixed prompt (then pass encoder_hidden_states=None)."""
        ehs = encoder_hidden_states.to(self.device).contiguous()
        self._ctx_keepalive = ehs
        t = L.as_tensor(ehs)
        L.check(L.lib().mrisr_model_set_context(self._h, C.byref(t), int(latent_hw[0]), int(latent_hw[1]), L.stream_ptr()))


class ControlNetModel(_DeviceModel):
    _create = "mrisr_controlnet_create"

    def __call__(self, sample: torch.Tensor, timestep, encoder_hidden_states: Optional[torch.Tensor] = None,
                 controlnet_cond: Optional[torch.Tensor] = None, conditioning_scale: float = 1.0,
                 return_dict: bool = True, rows: Optional[Tuple[int, int]] = None, **_unused):
        """``rows=(lo, hi)``: a forward on the row window [lo, hi) of the planned batch, as ``UNet2DConditionModel``'s: ``sample`` carries the
        window's rows, ``encoder_hidden_states`` and ``controlnet_cond`` must be None (both are the ones cached for the full batch) and
        ``conditioning_scale`` 1."""
        if not self._finalized:
            raise L.MrisrError("load_state_dict() first")
        sample = sample.to(self.device).contiguous()
        B, _, h, w = sample.shape
        rows = _check_rows(rows, B, encoder_hidden_states is not None or controlnet_cond is not None)
        if rows is not None and conditioning_scale != 1.0:
            raise ValueError("rows=(lo, hi): conditioning_scale must be 1")
        t = self._timestep(timestep, B)
        ehs = encoder_hidden_states.to(self.device).contiguous() if encoder_hidden_states is not None else None
        cond = controlnet_cond.to(self.device).contiguous() if controlnet_cond is not None else None
        if cond is not None and (cond.shape[2] != 8 * h or cond.shape[3] != 8 * w):
            raise ValueError(f"controlnet_cond must be [B,3,{8 * h},{8 * w}]; got {tuple(cond.shape)}")
        shapes = self._skip_shapes(B, h, w)
        outs = [torch.empty(s, dtype=sample.dtype, device=self.device) for s in shapes]
        d_arr = L.tensor_array([L.as_tensor(o) for o in outs[:-1]])
        t_mid = L.as_tensor(outs[-1])
        t_s, t_t = L.as_tensor(sample), L.as_tensor(t)
        t_e = L.as_tensor(ehs) if ehs is not None else None
        t_c = L.as_tensor(cond) if cond is not None else None
        if rows is not None:
            L.check(L.lib().mrisr_model_forward_rows(self._h, rows[0], rows[1], C.byref(t_s), C.byref(t_t), d_arr, len(outs) - 1, C.byref(t_mid),
                                                     None, 0, None, L.stream_ptr()))
        else:
            L.check(L.lib().mrisr_controlnet_forward(self._h, C.byref(t_s), C.byref(t_t), C.byref(t_e) if t_e else None,
                                                     C.byref(t_c) if t_c else None, C.c_float(conditioning_scale), d_arr,
                                                     len(outs) - 1, C.byref(t_mid), L.stream_ptr()))
        if return_dict:
            return _ControlNetOutput(outs[:-1], outs[-1])
        return outs[:-1], outs[-1]


class Adapter_XL:
    """T2I-Adapter of the reference (``src/adapters/modules.py:114-157``).  Only ``sk=True`` is runnable in the
    reference; ``sk=False`` raises here too."""

    def __init__(self, channels=(320, 640, 1280, 1280), nums_rb=3, cin=192, ksize=3, sk=True, use_conv=True,
                 compute_dtype="bf16", device="cuda"):
        if not sk:
            raise RuntimeError("Adapter_XL(sk=False) cannot run in the reference either: the skep conv is applied to the "
                               "already-projected tensor (channel mismatch). Use sk=True.")
        if not torch.cuda.is_available():
            raise L.MrisrError("mrisr needs an AMD GPU (gfx950); there is no CPU fallback")
        self.channels, self.nums_rb, self.cin, self.ksize, self.use_conv = tuple(channels), nums_rb, cin, ksize, use_conv
        self.device = torch.device(device)
        self.compute_dtype = L.torch_dtype(L.dtype_id(compute_dtype))
        c = L.AdapterCfg()
        for i, ch in enumerate(channels):
            c.channels[i] = ch
        c.nums_rb, c.cin, c.ksize, c.use_conv = nums_rb, cin, ksize, 1 if use_conv else 0
        c.compute_dtype = L.dtype_id(compute_dtype)
        self._h = C.c_void_p()
        L.check(L.lib().mrisr_adapter_create(C.byref(c), C.byref(self._h)))
        self._params: Dict[str, torch.Tensor] = {}
        self._finalized = False

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                L.lib().mrisr_adapter_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def eval(self):
        return self

    def state_dict(self):
        return dict(self._params)

    def load_state_dict(self, sd, strict: bool = True):
        fn = L.lib().mrisr_adapter_set_param
        for k, v in sd.items():
            self._params[k] = v
            L.push_param(fn, self._h, k, v)
        L.check(L.lib().mrisr_adapter_finalize(self._h, L.stream_ptr()))
        self._finalized = True
        return self

    def feature_shapes(self, B: int, H: int, W: int):
        h, w = H // 8, W // 8
        return [(B, c, h >> i, w >> i) for i, c in enumerate(self.channels)]

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        if not self._finalized:
            raise L.MrisrError("load_state_dict() first")
        assert x.shape[1] * 64 == self.cin  # same shape guard family as modules.py:71,75
        x = x.to(self.device).contiguous()
        B, _, H, W = x.shape
        feats = [torch.empty(s, dtype=x.dtype, device=self.device) for s in self.feature_shapes(B, H, W)]
        arr = L.tensor_array([L.as_tensor(f) for f in feats])
        t_x = L.as_tensor(x)
        L.check(L.lib().mrisr_adapter_forward(self._h, C.byref(t_x), arr, len(feats), L.stream_ptr()))
        return feats

    __call__ = forward
