"""``mrisr.fit``: the reference's LoRA fine-tuning cell (notebook ResDif c11:14-41, batch preparation of
``src/adapters/res_srdiff.py:7-25``) as one call, with the step on the device.

Every item of the training set is VAE-encoded ONCE; its posterior moments stay on the device.  One optimiser step is then
``gradient_accumulation_steps`` replays of graph M (batch builder -> forward / loss / backward into the flat gradient) and one replay
of graph O (clip + AdamW + EMA from per-step device tables, adapter re-pack, loss / grad-norm / lr rings) - see ``csrc/fit.hip``.
The host does not synchronise inside a step; it reads the rings every ``logging_steps``.  Random numbers are Philox keyed by
(seed, step, micro-batch, sample, element, stream), so a batch is a pure function of (seed, step, micro-batch): a resumed run
draws exactly the batches the uninterrupted run would have drawn.

    for s in range(max_train_steps):                       # what the graphs replace, per optimiser step
        for k in range(gradient_accumulation_steps):
            z_hr, z_lr = posterior samples * scaling_factor of the batch's items
            t ~ U[0, T), eps ~ N(0, 1); noisy = get_res_shifting_latents(z_hr, z_lr, t, scheduler, eps)
            ehs = caption embedding, or the "" embedding with probability proportion_empty_prompts
            loss_k = mse(unet(noisy, t, ehs), eps); grad += d loss_k
        clip_grad_norm_(max_grad_norm) of grad / (world * accum); AdamW(lr = schedule(s)); EMA(decay(s + 1)); grad = 0

With ``adapter=`` (the notebook's T2I-Adapter run, ``lora_rank: null``) each micro-batch also builds the condition (the item's LR
image, 3 channels, PixelUnshuffle(8)), runs the adapter, adds its features inside the UNet and differentiates the adapter with the
feature gradients; the clip then takes the joint norm of the LoRA bucket (if the UNet trains) and the adapter bucket, as
``joint_step`` does.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .config import TrainConfig, log_configs
from .dist import all_reduce_sum_, shard_range
from .train import AdapterTrainer, LoRATrainer, _FlatAdamW, cosine_lr

LR_SCHEDULERS = ("cosine", "constant")
WEIGHTS_NAME = "pytorch_lora_weights.safetensors"
ADAPTER_NAME = "t2i_adapter.safetensors"
STATE_NAME = "fit_state.json"


class _FitConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "accum", "max_steps", "world", "sample_base", "n_items", "latent_channels",
                                         "latent_h", "latent_w", "n_captions", "ctx_len", "ctx_dim", "empty_row",
                                         "num_train_timesteps", "use_ema")] + \
               [(n, C.c_float) for n in ("proportion_empty", "scaling_factor", "beta1", "beta2", "eps", "weight_decay",
                                         "max_grad_norm")] + [("seed", C.c_uint64)]


class _FitAdapterArgs(C.Structure):
    _fields_ = [("adapter", C.c_void_p), ("cond", C.c_void_p), ("res", C.c_int32), ("exp_avg", C.c_void_p),
                ("exp_avg_sq", C.c_void_p), ("ema", C.c_void_p)]


# ---------------------------------------------------------------------------------------------- host-side tables (no GPU)
def check_config(config: TrainConfig, caption_embeds: Optional[Dict[str, torch.Tensor]] = None) -> None:
    """Everything ``fit`` refuses, checked before any GPU work."""
    if config.ddpm_scheduler_prediction_type != "epsilon":
        raise ValueError(f"fit trains epsilon prediction only; got prediction_type {config.ddpm_scheduler_prediction_type!r}")
    if config.lr_scheduler_name not in LR_SCHEDULERS:
        raise ValueError(f"lr_scheduler_name must be one of {LR_SCHEDULERS}; got {config.lr_scheduler_name!r}")
    if not 0.0 <= config.proportion_empty_prompts <= 1.0:
        raise ValueError("proportion_empty_prompts must lie in [0, 1]")
    if config.proportion_empty_prompts > 0 and caption_embeds is not None and "" not in caption_embeds:
        raise ValueError("proportion_empty_prompts > 0 needs the empty prompt's embedding under the key \"\" in caption_embeds")
    for k in ("max_train_steps", "train_batch_size", "gradient_accumulation_steps", "logging_steps", "validation_steps",
              "checkpointing_steps", "resolution"):
        if int(getattr(config, k)) < 1:
            raise ValueError(f"{k} must be >= 1")
    if config.lr_warmup_steps < 0:
        raise ValueError("lr_warmup_steps must be >= 0")


def check_validation_solver(validation_solver) -> None:
    """What ``fit(validation_solver=...)`` refuses, before any GPU work: anything but ``None`` or a multistep sampler kind."""
    if validation_solver is not None:
        from .pipeline import check_solver
        check_solver(validation_solver)


def check_validation_guidance(guidance_scale: float, guidance_rescale: float,
                              caption_embeds: Optional[Dict[str, torch.Tensor]]) -> bool:
    """What ``fit(validation_guidance_scale=..., validation_guidance_rescale=...)`` refuses, before any GPU work: the rules of
    ``Sampler.run``'s guidance, with ``caption_embeds[""]`` (what caption dropout trains on) as the unconditional embedding.
    Returns whether validation will sample with guidance."""
    from .pipeline import check_guidance
    shape = None
    if caption_embeds is not None and "" in caption_embeds:
        shape = (1,) + tuple(torch.as_tensor(caption_embeds[""]).shape[-2:])
    if float(guidance_scale) != 1.0 and shape is None:
        raise ValueError("validation_guidance_scale != 1 needs the empty prompt's embedding under the key \"\" in caption_embeds")
    return check_guidance(guidance_scale, guidance_rescale, shape if shape is not None else (1, 1, 1), shape, 1)


def trained_buckets(lora: bool, adapter: bool) -> List[str]:
    """The parameter sets a run trains, as ``fit_state.json`` records them."""
    return [b for b, on in (("lora", lora), ("adapter", adapter)) if on]


def check_resume_buckets(state: dict, buckets: List[str], path: str = "") -> None:
    """A checkpoint resumes only into a run that trains the same parameter sets; a state file without the field was written by a
    LoRA-only run."""
    have = list(state.get("buckets", ["lora"]))
    if sorted(have) != sorted(buckets):
        raise ValueError(f"checkpoint {path} trained {'+'.join(have)}; this run trains {'+'.join(buckets) or 'nothing'}")


def check_adapter(config: TrainConfig, unet, adapter) -> None:
    """What ``fit(adapter=...)`` refuses before the loop handle exists: the condition builder feeds ``cin = 192`` at ``resolution``,
    and the adapter's four features must land on the UNet's intrablock positions in the UNet's compute dtype."""
    res = int(config.resolution)
    if res % 8:
        raise ValueError(f"resolution {res} is not a multiple of 8: the adapter's PixelUnshuffle(8) needs one")
    if int(adapter.cin) != 192:
        raise ValueError(f"the condition builder feeds cin = 192 (3 channels, PixelUnshuffle(8)); the adapter has cin = {adapter.cin}")
    want = L.torch_dtype(L.dtype_id(config.compute_dtype()))
    if adapter.compute_dtype != want or adapter.compute_dtype != unet.compute_dtype:
        raise ValueError(f"mixed_precision={config.mixed_precision!r} means compute dtype {want}; the adapter computes in "
                         f"{adapter.compute_dtype}, the UNet in {unet.compute_dtype}")
    levels = tuple(unet.config.block_out_channels)
    if tuple(adapter.channels) != levels or adapter.nums_rb < 1:
        raise ValueError(f"the adapter's features {tuple(adapter.channels)} do not fit the UNet's intrablock positions {levels}")


def base_learning_rate(config: TrainConfig, world: int = 1) -> float:
    """``learning_rate``, times accumulation * batch * processes under ``scale_lr`` (diffusers' training scripts)."""
    lr = float(config.learning_rate)
    if config.scale_lr:
        lr *= config.gradient_accumulation_steps * config.train_batch_size * world
    return lr


def lr_table(config: TrainConfig, world: int = 1) -> List[float]:
    """Learning rate of optimiser step s (s from 0): the value the scheduler holds when ``optimizer.step()`` runs, i.e. before its
    own ``lr_scheduler.step()`` - ``cosine_lr(s, ...)`` for "cosine", the base rate for "constant" (diffusers ignores the warm-up there)."""
    base = base_learning_rate(config, world)
    n = int(config.max_train_steps)
    if config.lr_scheduler_name == "cosine":
        return [cosine_lr(s, base, int(config.lr_warmup_steps), n) for s in range(n)]
    if config.lr_scheduler_name == "constant":
        return [base] * n
    raise ValueError(f"lr_scheduler_name must be one of {LR_SCHEDULERS}; got {config.lr_scheduler_name!r}")


def ema_decay_table(max_steps: int, decay: float = 0.9999) -> List[float]:
    """EMA decay applied after optimiser step s: ``ema_decay_at(s + 1)`` (EMAModel counts its steps from 1)."""
    return [_FlatAdamW.ema_decay_at(s + 1, decay) for s in range(int(max_steps))]


def epoch_index_table(n_items: int, batch: int, world: int, rank: int, seed: int, n_micro: int) -> Tuple[np.ndarray, np.ndarray]:
    """Dataset item of every sample of this rank's first ``n_micro`` micro-batches, [n_micro, batch] int32, and the epoch of each
    micro-batch.  Epoch e shuffles all items with ``torch.randperm`` seeded (seed + e); rank r takes its ``shard_range`` of that
    permutation, cut to the same whole number of micro-batches on every rank (drop-last), so all ranks step through epochs in lock-step."""
    per_rank = (n_items // world) // batch
    if per_rank < 1:
        raise ValueError(f"{n_items} items do not fill one micro-batch of {batch} per rank on {world} rank(s)")
    rows, epochs, e = [], [], 0
    while len(rows) < n_micro:
        perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(int(seed) + e)).numpy()
        lo, hi = shard_range(n_items, world, rank)
        mine = perm[lo:hi][: per_rank * batch]
        for j in range(per_rank):
            rows.append(mine[j * batch:(j + 1) * batch])
            epochs.append(e)
        e += 1
    return np.ascontiguousarray(np.stack(rows[:n_micro]).astype(np.int32)), np.asarray(epochs[:n_micro], dtype=np.int64)


# ---------------------------------------------------------------------------------------------- the device loop
def _image(x, res: int, channels: int, dev) -> torch.Tensor:
    """One slice in [-1, 1] -> [channels, res, res] f32 on the device: 1 channel expanded (res_srdiff.py:49), resized when needed."""
    from .datasets import resize_slices
    x = torch.as_tensor(x).to(dev, torch.float32)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3:
        raise ValueError(f"dataset images must be [H, W] or [C, H, W]; got {tuple(x.shape)}")
    if tuple(x.shape[-2:]) != (res, res):
        x = resize_slices(x, (res, res))
    if x.shape[0] == 1 and channels != 1:
        x = x.expand(channels, -1, -1)
    return x.contiguous()


class FitLoop:
    """The C-ABI loop handle plus what it reads: the encoded training set, the caption table, the rings."""

    def __init__(self, config: TrainConfig, trainer: LoRATrainer, vae, train_dataset, caption_embeds: Dict[str, torch.Tensor],
                 world: int = 1, rank: int = 0, use_ema: bool = False, encode_batch: int = 16,
                 adapter_trainer: Optional[AdapterTrainer] = None):
        unet = trainer.unet
        dev = unet.device
        self.config, self.trainer, self.world, self.rank = config, trainer, int(world), int(rank)
        self.adapter_trainer = adapter_trainer
        if adapter_trainer is not None:
            check_adapter(config, unet, adapter_trainer.adapter)
            for k in ("betas", "eps", "weight_decay", "max_grad_norm"):
                if getattr(adapter_trainer, k) != getattr(trainer, k):
                    raise ValueError(f"one optimiser over both buckets: the adapter trainer's {k} differs from the UNet trainer's")
        B, accum, S = int(config.train_batch_size), int(config.gradient_accumulation_steps), int(config.max_train_steps)
        self.batch, self.accum, self.max_steps = B, accum, S
        # ---- encode every item once: posterior moments {HR mean, HR std, LR mean, LR std}, f32 on the device ----
        items = [train_dataset[i] for i in range(len(train_dataset))]
        if not items:
            raise ValueError("empty training set")
        res, cin = int(config.resolution), int(vae.config.in_channels)
        chunks = []
        with torch.no_grad():
            for i in range(0, len(items), encode_batch):
                part = items[i:i + encode_batch]
                mom = []
                for key in ("hr", "lr"):
                    x = torch.stack([_image(it[key], res, cin, dev) for it in part])
                    d = vae.encode(x).latent_dist
                    mom += [d.mean.float(), d.std.float()]
                chunks.append(torch.stack(mom, 1).reshape(len(part), 4, -1))
        self.moments = torch.cat(chunks).contiguous()
        if adapter_trainer is not None:
            # the condition of every item: its LR image at `resolution`, one channel (the kernel expands it to three)
            lrs = [_image(it["lr"], res, 1, dev) for it in items]
            if any(x.shape[0] != 1 for x in lrs):
                raise ValueError("the adapter's condition is built from 1-channel LR images")
            self.cond = torch.cat(lrs).contiguous()
        lat_c = int(vae.config.latent_channels)
        f = 2 ** (len(vae.config.block_out_channels) - 1)
        self.latent_shape = (lat_c, res // f, res // f)
        # ---- captions: one row per distinct prompt, every item points at its own ----
        names = list(caption_embeds)
        for it in items:
            if it["txt"] not in caption_embeds:
                raise KeyError(f"no caption embedding for prompt {it['txt']!r}")
        rows = [torch.as_tensor(caption_embeds[n]).reshape(-1, unet.config.cross_attention_dim) for n in names]
        if len({tuple(r.shape) for r in rows}) != 1:
            raise ValueError("caption embeddings must all be [L, D] of one L")
        self.captions = torch.stack(rows).to(dev, torch.float32).contiguous()
        cap_of_item = np.asarray([names.index(it["txt"]) for it in items], dtype=np.int32)
        empty_row = names.index("") if "" in names else -1
        # ---- tables ----
        self.index, self.epoch_of_micro = epoch_index_table(len(items), B, self.world, self.rank, config.seed, S * accum)
        self.lrs = np.asarray(lr_table(config, self.world), dtype=np.float32)
        self.decays = np.asarray(ema_decay_table(S), dtype=np.float32)
        from .schedulers import DDPMScheduler
        sched = DDPMScheduler(**config.scheduler_kwargs())
        ac = sched.alphas_cumprod.to(torch.float32).numpy().copy()
        self.loss_ring = torch.zeros(S, dtype=torch.float32, device=dev)
        self.grad_norm_ring = torch.zeros(S, dtype=torch.float32, device=dev)
        self.lr_ring = torch.zeros(S, dtype=torch.float32, device=dev)
        if use_ema and getattr(trainer, "ema", None) is None:
            trainer.ema_init()  # EMAModel(unet parameters) before the first step
        if use_ema and adapter_trainer is not None and getattr(adapter_trainer, "ema", None) is None:
            adapter_trainer.ema_init()
        self.use_ema = bool(use_ema)
        c = _FitConfig(batch=B, accum=accum, max_steps=S, world=self.world, sample_base=self.rank * B, n_items=len(items),
                       latent_channels=lat_c, latent_h=self.latent_shape[1], latent_w=self.latent_shape[2], n_captions=len(names),
                       ctx_len=self.captions.shape[1], ctx_dim=self.captions.shape[2], empty_row=empty_row,
                       num_train_timesteps=len(ac), use_ema=1 if use_ema else 0,
                       proportion_empty=float(config.proportion_empty_prompts), scaling_factor=float(vae.config.scaling_factor),
                       beta1=trainer.betas[0], beta2=trainer.betas[1], eps=trainer.eps, weight_decay=trainer.weight_decay,
                       max_grad_norm=float(trainer.max_grad_norm or 0.0), seed=int(config.seed) & (2 ** 64 - 1))
        self._c = c
        lib = L.lib()
        lib.mrisr_fit_destroy.restype = None
        lib.mrisr_fit_destroy.argtypes = [C.c_void_p]
        lib.mrisr_fit_get_step.argtypes = [C.c_void_p]
        lib.mrisr_fit_num_captures.argtypes = [C.c_void_p]
        self._h = C.c_void_p()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        args = (unet._h, C.byref(c), p(self.moments), p(self.captions), cap_of_item.ctypes.data_as(C.c_void_p),
                self.index.ctypes.data_as(C.c_void_p), ac.ctypes.data_as(C.c_void_p), self.lrs.ctypes.data_as(C.c_void_p),
                self.decays.ctypes.data_as(C.c_void_p), p(trainer.exp_avg), p(trainer.exp_avg_sq), p(trainer.ema) if use_ema else None,
                p(self.loss_ring), p(self.grad_norm_ring), p(self.lr_ring))
        if adapter_trainer is None:
            L.check(lib.mrisr_fit_create(*args, C.byref(self._h)))
        else:
            at = adapter_trainer
            self._ad = _FitAdapterArgs(adapter=at.adapter._h.value, cond=self.cond.data_ptr(), res=res, exp_avg=at.exp_avg.data_ptr(),
                                       exp_avg_sq=at.exp_avg_sq.data_ptr(), ema=at.ema.data_ptr() if use_ema else None)
            L.check(lib.mrisr_fit_create_adapter(*args, C.byref(self._ad), C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                L.lib().mrisr_fit_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @property
    def step(self) -> int:
        return int(L.lib().mrisr_fit_get_step(self._h))

    @property
    def num_captures(self) -> int:
        return int(L.lib().mrisr_fit_num_captures(self._h))

    def epoch(self, step: int) -> int:
        return int(self.epoch_of_micro[min(step, self.max_steps - 1) * self.accum])

    def _launch(self, fn, *args):
        """Graphs cannot be captured on the default stream: from there, run on this loop's own stream, fenced both ways by torch."""
        cur = torch.cuda.current_stream(self.moments.device)
        if cur.cuda_stream:
            return L.check(fn(self._h, *args, C.c_void_p(cur.cuda_stream)))
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.moments.device)
        self._side.wait_stream(cur)
        L.check(fn(self._h, *args, C.c_void_p(self._side.cuda_stream)))
        cur.wait_stream(self._side)

    def set_step(self, step: int):
        self._launch(L.lib().mrisr_fit_set_step, int(step))

    def micro(self):
        self._launch(L.lib().mrisr_fit_micro)

    def apply(self):
        self._launch(L.lib().mrisr_fit_apply)

    def make_batch(self, step: int, micro: int = 0) -> Dict[str, torch.Tensor]:
        """The batch graph M builds for (step, micro), eagerly: sample, timesteps, encoder_hidden_states, target, plus the posterior-
        sampling noise (eps_hr, eps_lr) and the caption row each sample got (caption_row)."""
        dev = self.moments.device
        B = self.batch
        lat = (B,) + self.latent_shape
        out = {"sample": torch.empty(lat, dtype=torch.float32, device=dev),
               "timesteps": torch.empty(B, dtype=torch.int64, device=dev),
               "encoder_hidden_states": torch.empty((B,) + tuple(self.captions.shape[1:]), dtype=torch.float32, device=dev),
               "target": torch.empty(lat, dtype=torch.float32, device=dev),
               "eps_hr": torch.empty(lat, dtype=torch.float32, device=dev),
               "eps_lr": torch.empty(lat, dtype=torch.float32, device=dev),
               "caption_row": torch.empty(B, dtype=torch.int32, device=dev)}
        p = {k: C.c_void_p(v.data_ptr()) for k, v in out.items()}
        L.check(L.lib().mrisr_fit_make_batch(self._h, int(step), int(micro), p["sample"], p["timesteps"], p["encoder_hidden_states"],
                                             p["target"], p["eps_hr"], p["eps_lr"], p["caption_row"], L.stream_ptr()))
        return out

    def make_condition(self, step: int, micro: int = 0, form: int = 0) -> torch.Tensor:
        """The adapter condition graph M builds for (step, micro), eagerly: form 0 is the [B, 3, res, res] f32 image (the input of
        ``Adapter_XL.forward``), form 1 the PixelUnshuffle(8) activation the graph feeds the adapter, [B, res/8, res/8, 192] NHWC
        in the compute dtype."""
        if self.adapter_trainer is None:
            raise ValueError("this loop trains no T2I-Adapter")
        dev, B, res = self.moments.device, self.batch, int(self.config.resolution)
        if form == 0:
            out = torch.empty((B, 3, res, res), dtype=torch.float32, device=dev)
        elif form == 1:
            out = torch.empty((B, res // 8, res // 8, 192), dtype=self.adapter_trainer.adapter.compute_dtype, device=dev)
        else:
            raise ValueError("form must be 0 (image) or 1 (unshuffled activation)")
        L.check(L.lib().mrisr_fit_make_condition(self._h, int(step), int(micro), C.c_void_p(out.data_ptr()), int(form), L.stream_ptr()))
        return out

    def item_indices(self, step: int, micro: int = 0) -> np.ndarray:
        return self.index[step * self.accum + micro]


@dataclass
class FitResult:
    trainer: LoRATrainer
    losses: np.ndarray                 # [max_train_steps] mean loss of each optimiser step (host copy of the ring)
    grad_norms: np.ndarray
    lrs: np.ndarray
    step: int
    metrics_path: Optional[str] = None
    validation_paths: List[str] = field(default_factory=list)
    checkpoint_paths: List[str] = field(default_factory=list)
    loop: Optional[FitLoop] = None
    adapter_trainer: Optional[AdapterTrainer] = None  # the trained T2I-Adapter (fit(adapter=...)); None otherwise


class _Accel:
    def __init__(self, device):
        self.device = device


def _world(process_group) -> Tuple[int, int]:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(process_group), dist.get_rank(process_group)
    if process_group is not None:
        raise ValueError("process_group given but torch.distributed is not initialised")
    return 1, 0


def fit(config: TrainConfig, unet, vae, train_dataset, caption_embeds: Dict[str, torch.Tensor], val_dataset=None, fixed_embeds=None,
        resume_from: Optional[str] = None, use_ema: bool = False, process_group=None, adapter=None,
        validation_guidance_scale: float = 1.0, validation_guidance_rescale: float = 0.0,
        validation_solver: Optional[str] = None) -> FitResult:
    """LoRA fine-tuning of ``unet`` (created with ``lora_rank > 0, lora_fused=True`` and loaded) on ``train_dataset`` (items
    ``{'hr', 'lr', 'txt'}``, images in [-1, 1]); ``caption_embeds[txt]`` is the [L, D] text embedding of each prompt ("" for the
    dropped caption).  Writes ``output_dir/metrics.jsonl``, ``validation/step-N.png`` (with ``val_dataset``) and
    ``checkpoint-N/``; ``resume_from`` is such a checkpoint directory.  ``adapter``: a loaded ``Adapter_XL`` trained as well,
    conditioned on each item's LR image; with a ``lora_rank=0`` UNet it is the only thing trained (the UNet is frozen).
    ``validation_guidance_scale`` / ``validation_guidance_rescale``: the validation panels are sampled with classifier-free guidance
    against ``caption_embeds[""]`` (``log_validation``); the defaults sample as before.  ``validation_solver`` ("unipc" /
    "dpmsolver++"): the panels are sampled with that LR-anchored deterministic multistep solver (order 2, "zero" final point) and no
    step noise is drawn; ``None`` keeps the reference's stochastic sampler."""
    check_config(config, caption_embeds)
    check_validation_solver(validation_solver)
    guided = check_validation_guidance(validation_guidance_scale, validation_guidance_rescale, caption_embeds)
    guidance = (float(validation_guidance_scale), float(validation_guidance_rescale)) if guided else None
    # the whole run on one side stream: graph launches, the all-reduce between them, ring reads, checkpoints and validation are then
    # ordered by the stream itself (the library fences the legacy default stream through an internal one otherwise)
    side = torch.cuda.Stream(device=unet.device)
    side.wait_stream(torch.cuda.current_stream(unet.device))
    with torch.cuda.stream(side):
        res = _fit(config, unet, vae, train_dataset, caption_embeds, val_dataset, fixed_embeds, resume_from, use_ema, process_group,
                   adapter, guidance, validation_solver)
    torch.cuda.current_stream(unet.device).wait_stream(side)
    return res


def _fit(config, unet, vae, train_dataset, caption_embeds, val_dataset, fixed_embeds, resume_from, use_ema, process_group,
         adapter=None, guidance=None, validation_solver=None) -> FitResult:
    want = L.torch_dtype(L.dtype_id(config.compute_dtype()))
    if unet.compute_dtype != want:
        raise ValueError(f"mixed_precision={config.mixed_precision!r} means compute dtype {want}; the UNet computes in {unet.compute_dtype}")
    lora = bool(getattr(unet, "lora_rank", 0))
    if not lora and adapter is None:
        raise ValueError("the UNet has no LoRA (lora_rank=0) and no adapter was given: nothing to train")
    if adapter is not None:
        if not getattr(adapter, "_finalized", False):
            raise ValueError("load the adapter's weights first (Adapter_XL.load_state_dict)")
        check_adapter(config, unet, adapter)
    buckets = trained_buckets(lora, adapter is not None)
    world, rank = _world(process_group)
    opt = {**config.optimizer_kwargs(), "lr": base_learning_rate(config, world)}
    trainer = LoRATrainer(unet, **opt, process_group=process_group)
    atr = AdapterTrainer(adapter, **opt, process_group=process_group) if adapter is not None else None
    S = int(config.max_train_steps)
    start, state = 0, None
    if resume_from is not None:
        with open(os.path.join(resume_from, STATE_NAME)) as fh:
            state = json.load(fh)
        if int(state["seed"]) != int(config.seed):
            raise ValueError(f"checkpoint {resume_from} was written by a run with seed {state['seed']}, not {config.seed}")
        check_resume_buckets(state, buckets, resume_from)
        # before the loop handle: it binds the EMA vectors' addresses
        if lora:
            trainer.load_checkpoint(os.path.join(resume_from, WEIGHTS_NAME))
        if atr is not None:
            atr.load_checkpoint(os.path.join(resume_from, ADAPTER_NAME))
        start = int(state["step"])
    loop = FitLoop(config, trainer, vae, train_dataset, caption_embeds, world, rank, use_ema, adapter_trainer=atr)
    if state is not None:
        for ring, key in ((loop.loss_ring, "losses"), (loop.grad_norm_ring, "grad_norms"), (loop.lr_ring, "lrs")):
            ring[:start].copy_(torch.tensor(state[key][:start], dtype=torch.float32))
    loop.set_step(start)

    out = config.output_dir
    writer = rank == 0
    metrics_path = os.path.join(out, "metrics.jsonl")
    if writer:
        os.makedirs(out, exist_ok=True)
        with open(metrics_path, "a") as fh:
            fh.write(json.dumps(log_configs(config), default=str) + "\n")
    res = FitResult(trainer, np.zeros(S, np.float32), np.zeros(S, np.float32), np.zeros(S, np.float32), start,
                    metrics_path if writer else None, loop=loop, adapter_trainer=atr)
    val_batch = None
    if val_dataset is not None:
        it = val_dataset[0]
        hr, lr = (_image(it[k], int(config.resolution), 1, unet.device)[:1][None] for k in ("hr", "lr"))
        val_batch = {"hr": hr, "lr": lr}
        if fixed_embeds is None:
            txt = it.get("txt", "") if isinstance(it, dict) else ""
            fixed_embeds = torch.as_tensor(caption_embeds[txt] if txt in caption_embeds else next(iter(caption_embeds.values())))
        fixed_embeds = fixed_embeds.reshape(-1, *fixed_embeds.shape[-2:]).to(unet.device, torch.float32)
    val_kw = {}
    if validation_solver is not None:
        val_kw["solver"] = validation_solver
    if guidance is not None:  # classifier-free guidance against the embedding the caption dropout trained on
        empty = torch.as_tensor(caption_embeds[""])
        val_kw.update(guidance_scale=guidance[0], guidance_rescale=guidance[1],
                      uncond_embeds=empty.reshape(-1, *empty.shape[-2:]).to(unet.device, torch.float32))

    samples = config.train_batch_size * config.gradient_accumulation_steps * world
    t_log, last_log = time.perf_counter(), start
    for s in range(start, S):
        for _ in range(config.gradient_accumulation_steps):
            loop.micro()
        if world > 1:
            if lora:
                all_reduce_sum_(trainer.grad, process_group)
            if atr is not None:
                all_reduce_sum_(atr.grad, process_group)
        loop.apply()
        step = s + 1
        for t in (trainer, atr):
            if t is not None:
                t.step_count = step
                if use_ema:
                    t.ema_steps = step
        if step % config.logging_steps == 0 or step == S:
            window = slice(last_log, step)
            loss, gn, lr = (r[window].cpu() for r in (loop.loss_ring, loop.grad_norm_ring, loop.lr_ring))  # the one sync of the window
            now = time.perf_counter()
            if writer and step % config.logging_steps == 0:
                line = {"step": step, "epoch": loop.epoch(s), "loss": float(loss.mean()), "lr": float(lr[-1]), "grad_norm": float(gn[-1]),
                        "ema_decay": float(loop.decays[s]) if use_ema else None,
                        "samples_per_s": samples * (step - last_log) / max(now - t_log, 1e-9)}
                with open(metrics_path, "a") as fh:
                    fh.write(json.dumps(line) + "\n")
            t_log, last_log = now, step
        if val_batch is not None and step % config.validation_steps == 0 and writer:
            from .pipeline import log_validation
            from .schedulers import DDPMScheduler
            panel = log_validation(unet, None, vae, [val_batch], DDPMScheduler(**config.scheduler_kwargs()), torch.float32,
                                   _Accel(unet.device), fixed_embeds, adapter=adapter, **val_kw)
            os.makedirs(os.path.join(out, "validation"), exist_ok=True)
            path = os.path.join(out, "validation", f"step-{step}.png")
            panel.save(path)
            res.validation_paths.append(path)
        if step % config.checkpointing_steps == 0 and writer:
            res.checkpoint_paths.append(_save(out, step, config, trainer, loop, use_ema, atr, buckets))
    torch.cuda.current_stream().synchronize()
    res.losses, res.grad_norms, res.lrs = (r.cpu().numpy() for r in (loop.loss_ring, loop.grad_norm_ring, loop.lr_ring))
    res.step = loop.step
    return res


def _save(out: str, step: int, config: TrainConfig, trainer: LoRATrainer, loop: FitLoop, use_ema: bool,
          adapter_trainer: Optional[AdapterTrainer] = None, buckets: Optional[List[str]] = None) -> str:
    d = os.path.join(out, f"checkpoint-{step}")
    os.makedirs(d, exist_ok=True)
    buckets = buckets or ["lora"]
    if "lora" in buckets:
        trainer.save_checkpoint(os.path.join(d, WEIGHTS_NAME))  # peft keys; moments and EMA in the .optim.pt next to it
        if use_ema:
            trainer.save_checkpoint(os.path.join(d, "ema_" + WEIGHTS_NAME), use_ema=True)
    if adapter_trainer is not None:
        adapter_trainer.save_checkpoint(os.path.join(d, ADAPTER_NAME))  # the reference module's own keys (Adapter_XL state dict)
        if use_ema:
            adapter_trainer.save_checkpoint(os.path.join(d, "ema_" + ADAPTER_NAME), use_ema=True)
    state = {"step": step, "seed": int(config.seed),
             "losses": loop.loss_ring[:step].cpu().tolist(), "grad_norms": loop.grad_norm_ring[:step].cpu().tolist(),
             "lrs": loop.lr_ring[:step].cpu().tolist()}
    if adapter_trainer is not None:
        state["buckets"] = buckets  # LoRA-only runs write the file as before: no field means LoRA-only
    with open(os.path.join(d, STATE_NAME), "w") as fh:
        json.dump(state, fh)
    return d
