/* mrisr.h - C ABI of libmrisr.so: the MI355X (gfx950) denoiser hot path of
 * Bernat-C/MRI-Diffusion-SuperResolution, behind the call surface the reference uses.
 *
 * What each entry point replaces in the reference (file:line under /root/reference):
 *   mrisr_unet_forward        <- unet(latents, t, encoder_hidden_states=..., down_block_additional_residuals=...,
 *                                     mid_block_additional_residual=...).sample      src/adapters/res_srdiff.py:73-78
 *                                (diffusers UNet2DConditionModel; + down_intrablock_additional_residuals for T2I-Adapter)
 *   mrisr_controlnet_forward  <- controlnet(latents, t, encoder_hidden_states=..., controlnet_cond=...,
 *                                     return_dict=False)                             src/adapters/res_srdiff.py:65-70
 *   mrisr_adapter_forward     <- Adapter_XL.forward                                  src/adapters/modules.py:146-157
 *   mrisr_resshift_forward    <- get_res_shifting_latents                            src/adapters/res_srdiff.py:7-25
 *   mrisr_sampler_*           <- the timestep loop of log_validation                 src/adapters/res_srdiff.py:63-96
 *                                (Res-SRDiff reverse step :84-96, or the DDIM(eta=0) step BASELINE.json names)
 *   mrisr_*_set_param         <- nn.Module.load_state_dict with diffusers / peft / reference key names
 *
 * Conventions
 *   - every function returns 0 on success; otherwise mrisr_last_error() (thread-local) describes the failure.
 *   - all tensors are caller-owned DEVICE memory described by mrisr_tensor (contiguous; NCHW like torch unless
 *     layout says NHWC).  Kernels are enqueued on the caller's stream; nothing synchronises internally, and
 *     nothing allocates inside *_forward after the first call for a given shape (hipGraph-capturable).
 *   - a handle is bound to the device that was current at creation; handles are not thread-safe.
 *   - no torch / C++ types cross this boundary.
 */
#ifndef MRISR_H
#define MRISR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MRISR_F32 = 0, MRISR_BF16 = 1, MRISR_F16 = 2, MRISR_I64 = 3 } mrisr_dtype;
typedef enum { MRISR_NCHW = 0, MRISR_NHWC = 1 } mrisr_layout;

typedef struct {
    void* data;        /* device pointer (host pointer only where a function says so) */
    int32_t dtype;     /* mrisr_dtype */
    int32_t layout;    /* mrisr_layout; ignored for ndim < 4 */
    int32_t ndim;
    int64_t shape[4];  /* logical NCHW order for 4-D image tensors: {B, C, H, W} */
} mrisr_tensor;

/* Mirror of the diffusers config keys the path depends on (SD-1.5 values in comments). */
typedef struct {
    int32_t in_channels;            /* 4 */
    int32_t out_channels;           /* 4 */
    int32_t num_levels;             /* 4 */
    int32_t block_out_channels[4];  /* 320, 640, 1280, 1280 */
    int32_t attn_levels[4];         /* 1, 1, 1, 0  (CrossAttn{Down,Up}Block2D at that level) */
    int32_t layers_per_block;       /* 2 */
    int32_t num_heads;              /* 8 (diffusers "attention_head_dim": 8) */
    int32_t cross_attention_dim;    /* 768 */
    int32_t norm_num_groups;        /* 32 */
    float norm_eps;                 /* 1e-5 */
    int32_t cond_channels;          /* ControlNet: 3 */
    int32_t cond_embed_channels[4]; /* ControlNet: 16, 32, 96, 256 */
    int32_t compute_dtype;          /* MRISR_BF16 (fast: bf16 storage, f32 accumulate/statistics) or
                                       MRISR_F32 (parity: f32 storage, exact-f32 MFMA) */
    int32_t lora_rank;              /* 0 = no LoRA; else rank of the peft adapters that will be set */
    int32_t lora_fused;             /* 1: rank-r tail fused into the projection GEMMs; 0: merged into W at finalize */
    int32_t flash_attention;        /* 1: fused flash kernel (bf16 only); 0: materialised scores */
    int32_t fp8_linears;            /* 0: off; 1: K = 320 projections; 2: K = 320 and 640 (bf16 models): these projections of the transformer blocks - incl. the LoRA
                                       targets to_q/k/v, to_out - run with OCP e4m3 operands on the fp8 MFMA (per-output-channel
                                       weight scales, per-row activation scales computed in-kernel), f32 accumulate; BASELINE configs[4] */
    int32_t fp8_attention;          /* 1 (bf16 models, flash_attention): Q K^T and P V of every attention on the fp8 MFMA (OCP e4m3 operands,
                                       per-head scales, f32 softmax and accumulate); the log-sum-exp kept for the backward is unchanged */
    int32_t fp8_train;              /* 1: mrisr_train_step runs its FORWARD with the fp8 projections / fp8 attention selected above
                                       and its backward in bf16 with f32 accumulation, straight through the quantisers ("mixed-precision
                                       training" of BASELINE configs[4]); 0: the training forward stays bf16 whatever the inference mode is */
} mrisr_unet_cfg;

typedef struct mrisr_model mrisr_model; /* UNet2DConditionModel or ControlNetModel */
typedef struct mrisr_adapter mrisr_adapter;
typedef struct mrisr_sampler mrisr_sampler;

const char* mrisr_last_error(void);
const char* mrisr_version(void);

/* ---- model lifetime & weights ---------------------------------------------------------------- */
int mrisr_unet_create(const mrisr_unet_cfg* cfg, mrisr_model** out);
int mrisr_controlnet_create(const mrisr_unet_cfg* cfg, mrisr_model** out);
void mrisr_model_destroy(mrisr_model* m);
/* key: diffusers state-dict name, peft LoRA name (<module>.lora_A.default.weight /
 * lora_B.default.weight; <module>.base_layer.weight accepted for wrapped layers).  data: f32, host or device
 * (is_device), contiguous, torch shape.  Copied; the caller may free it afterwards. */
int mrisr_model_set_param(mrisr_model* m, const char* key, const float* data, const int64_t* shape, int ndim,
                          int is_device);
int mrisr_model_set_lora_scale(mrisr_model* m, float scale); /* lora_alpha / r */
/* use_dora != 0: a DoRA handle (peft use_dora=True).  Every linear that carries lora_A / lora_B must then carry
 * <module>.lora_magnitude_vector.default.weight [out_features] too, and computes y = b + m / ||W + s B A||_row o (x W^T + s (x A^T) B^T).
 * Linear targets of a UNet handle only; not with the fp8 modes.  Call before mrisr_model_finalize. */
int mrisr_model_set_dora(mrisr_model* m, int use_dora);
/* Perturbed-attention guidance state of a UNet handle (contract: "perturbed-attention guidance" below).  Until it is cleared, every
 * mrisr_unet_forward treats samples first_sample .. first_sample + n_samples - 1 of its batch as PERTURBED: in transformer block i (forward
 * order: down blocks, mid, up blocks; i < mrisr_model_num_transformer_blocks) with bit i of block_mask set, their attn1 returns
 * to_out.0(to_v(norm1(h))) - the attention map is the identity.  The other samples, attn2, the feed-forward and the other blocks are
 * untouched.  n_samples == 0 or block_mask == 0 clears the state.  Refused: a ControlNet handle, a UNet built with fp8_attention, a mask
 * bit beyond the last block; a forward whose batch does not hold the range, a cached forward (mrisr_unet_forward_cached) and a training
 * step are refused while the state is set.  The workspace is planned per state.  mrisr_sampler_run_pag sets and clears it itself. */
int mrisr_model_set_pag(mrisr_model* m, uint32_t block_mask, int first_sample, int n_samples);
/* FreeU state of a UNet handle (contract: "FreeU" below; diffusers' UNet2DConditionModel.enable_freeu(s1, s2, b1, b2)).  While on,
 * every mrisr_unet_forward and every sampler step on the handle applies, in each resnet stage of up block k in {0, 1} (forward order;
 * stage 0 takes (b1, s1), stage 1 takes (b2, s2); an up block the UNet does not have is skipped) and before hidden and skip are
 * concatenated:  hidden[:, :Ch / 2] *= b   and   skip = fourier_filter(skip, threshold = 1, scale = s).  on == 0 clears the state (the
 * four values are ignored) and leaves the forward as it was: same launches, same workspace, same bits.  Refused: a ControlNet handle, a
 * value that is negative or not finite; mrisr_unet_forward_cached, a sampler run with a cache interval > 1, mrisr_sampler_set_cache with
 * interval > 1 and a training step are refused while the state is on.  The state is part of the workspace key and of the sampler's graph
 * key: a change plans and captures again. */
int mrisr_model_set_freeu(mrisr_model* m, int on, float s1, float s2, float b1, float b2);
/* Re-lays weights out for the kernels (NHWC filter order, fused QKV, GEGLU interleave, LoRA tails, ...).
 * Must be called after the last set_param and before forward; may be called again after updating params. */
int mrisr_model_finalize(mrisr_model* m, void* stream);
int64_t mrisr_model_num_params(const mrisr_model* m);
int64_t mrisr_model_workspace_bytes(const mrisr_model* m);

/* ---- UNet2DConditionModel.forward ------------------------------------------------------------- */
/* sample [B,Cin,h,w]; timestep: device int64, ndim 0 (broadcast) or [B]; ehs [B,L,Dctx] or NULL to reuse the
 * projections cached by the previous call / mrisr_model_set_context; down_res: 0 or 12(=n_skips) tensors shaped like
 * the skips; mid_res: NULL or [B,C_mid,h/8,w/8]; intrablock: 0 or num_levels tensors (T2I-Adapter features);
 * out [B,Cout,h,w] in out->dtype. */
int mrisr_unet_forward(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep,
                       const mrisr_tensor* ehs, const mrisr_tensor* down_res, int n_down_res,
                       const mrisr_tensor* mid_res, const mrisr_tensor* intrablock, int n_intrablock,
                       mrisr_tensor* out, void* stream);
/* Pre-compute the cross-attention K/V projections of a fixed prompt embedding (timestep-invariant). */
int mrisr_model_set_context(mrisr_model* m, const mrisr_tensor* ehs, int latent_h, int latent_w, void* stream);
int mrisr_model_num_skips(const mrisr_model* m);
/* transformer blocks of the handle, in forward order: down_blocks.i.attentions.j, mid_block.attentions.0, up_blocks.i.attentions.j (16 for SD-1.5) */
int mrisr_model_num_transformer_blocks(const mrisr_model* m);
/* shape {B,C,H,W} of skip k for a latent of h x w (k == num_skips -> the mid block tensor) */
int mrisr_model_skip_shape(const mrisr_model* m, int k, int B, int h, int w, int64_t shape[4]);

/* ---- feature cache (DeepCache, Ma et al. 2023): one forward ------------------------------------- */
/* The encoder hands the decoder the skips s_0 .. s_{n-1} (n = mrisr_model_num_skips); decoder stage q = 0 .. n-1 (one up-block
 * resnet + its transformer) consumes s_{n-1-q}.  For 1 <= depth <= n-1 the cache is the input x of stage n-1-depth: the tensor
 * concatenated with s_depth, after any upsampler conv before that stage.  shape {B,C,H,W} of it for a latent of h x w: */
int mrisr_unet_cache_shape(const mrisr_model* m, int depth, int B, int h, int w, int64_t shape[4]);
/* mrisr_unet_forward without ControlNet residuals, with `cache`: a caller tensor of exactly mrisr_unet_cache_shape, layout NHWC, the
 * compute dtype.  shallow == 0: the ordinary forward, which also WRITES cache.  shallow == 1: READS it - time embedding, conv_in and
 * the encoder up to the producer of s_depth (adapter features that land in s_0 .. s_depth are added, deeper ones ignored), no mid
 * block, decoder stages n-1-depth .. n-1 starting from cache, conv_norm_out, conv_out.  A shallow forward fed the cache of a full
 * forward of the same (sample, timestep, ehs) reproduces its output. */
int mrisr_unet_forward_cached(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                              const mrisr_tensor* intrablock, int n_intrablock, int depth, int shallow, mrisr_tensor* cache,
                              mrisr_tensor* out, void* stream);

/* ---- ControlNetModel.forward ------------------------------------------------------------------- */
/* cond [B,3,8h,8w] or NULL to reuse the cached condition embedding; down_out: n_skips tensors, mid_out: 1. */
int mrisr_controlnet_forward(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep,
                             const mrisr_tensor* ehs, const mrisr_tensor* cond, float conditioning_scale,
                             mrisr_tensor* down_out, int n_down_out, mrisr_tensor* mid_out, void* stream);
int mrisr_controlnet_set_cond(mrisr_model* m, const mrisr_tensor* cond, void* stream);

/* ---- a forward on a row window of the planned batch ------------------------------------------------
 * Rows [row_lo, row_hi) of the batch the handle's workspace is planned for (by a forward, mrisr_model_set_context or a sampler run), in the
 * same workspace: nothing is planned again, and a full-batch forward afterwards finds its workspace as it left it.  `sample` carries
 * row_hi - row_lo rows at the planned h, w; the context - and a ControlNet's condition image - are the ones cached for the full batch, read at
 * the window's rows.  UNet handle: down (n_down tensors, or NULL / 0), mid (or NULL) and the n_intrablock features are inputs that carry the
 * window's rows; `out` receives the prediction.  ControlNet handle: down (n_skips tensors) and mid are the outputs; no features, out NULL.
 * A window must not contain perturbed samples (mrisr_model_set_pag), runs the whole network (no feature cache) and is refused while a
 * training forward is being recorded.  The sampler's reduced steps (mrisr_sampler_set_skip) run through the same path. */
int mrisr_model_forward_rows(mrisr_model* m, int row_lo, int row_hi, const mrisr_tensor* sample, const mrisr_tensor* timestep, mrisr_tensor* down,
                             int n_down, mrisr_tensor* mid, const mrisr_tensor* intrablock, int n_intrablock, mrisr_tensor* out, void* stream);

/* ---- T2I-Adapter (Adapter_XL, sk=True) ----------------------------------------------------------- */
typedef struct {
    int32_t channels[4]; /* 320, 640, 1280, 1280 */
    int32_t nums_rb;     /* 3 */
    int32_t cin;         /* 192 = 3*8*8 */
    int32_t ksize;       /* 3 (1 also supported) */
    int32_t use_conv;    /* 1: stride-2 conv downsample */
    int32_t compute_dtype;
} mrisr_adapter_cfg;
int mrisr_adapter_create(const mrisr_adapter_cfg* cfg, mrisr_adapter** out);
void mrisr_adapter_destroy(mrisr_adapter* a);
int mrisr_adapter_set_param(mrisr_adapter* a, const char* key, const float* data, const int64_t* shape, int ndim,
                            int is_device);
int mrisr_adapter_finalize(mrisr_adapter* a, void* stream);
/* x [B,3,8h,8w] -> 4 feature maps (caller-allocated, any dtype/layout) */
int mrisr_adapter_forward(mrisr_adapter* a, const mrisr_tensor* x, mrisr_tensor* feats, int n_feats, void* stream);

/* ---- scheduler math (f32 latents, elementwise) --------------------------------------------------- */
/* x_t = sqrt(a_t) HR + (1-sqrt(a_t)) LR + sqrt(1-a_t) eps, a_t = alphas_cumprod[t]; t: device int64 0-dim or [B] */
int mrisr_resshift_forward(const mrisr_tensor* hr, const mrisr_tensor* lr, const mrisr_tensor* noise,
                           const float* alphas_cumprod_dev, const mrisr_tensor* timestep, mrisr_tensor* out,
                           void* stream);

/* ---- sampler: the timestep loop, one hipGraph per step -------------------------------------------- */
/* MRISR_STEP_DDPM: the ancestral step of diffusers' DDPMScheduler.step ("fixed_small" variance; BASELINE config 1, "10-step
 * DDPM"): t_prev = t - T/n, alpha_t = abar_t / abar_prev, x0 = (x - sqrt(1-abar_t) eps) / sqrt(abar_t) [clipped to
 * +-clip_sample_range when set], x_prev = sqrt(abar_prev) (1-alpha_t)/(1-abar_t) x0 + sqrt(alpha_t) (1-abar_prev)/(1-abar_t) x
 * + sqrt((1-abar_prev)/(1-abar_t) (1-alpha_t)) z for t > 0;  z = step_noise slab i (NULL: the mean only). */
/* MRISR_STEP_UNIPC / MRISR_STEP_DPMSOLVERPP: deterministic linear multistep solvers in data prediction - UniPC with the bh2 variant
 * (Zhao et al. 2023) and DPM-Solver++ 2M, midpoint (Lu et al. 2022) - on the grid t_0 > ... > t_{n-1} of `timesteps`, then a final
 * point.  The papers' algorithms on this table; not pinned to diffusers (which is not available to this project).  The sampler owns
 * a ring of solver_order x0 predictions and, for UniPC, the previous corrected state; both are zeroed at the start of every run.
 * With lr_latents the solver integrates z = x - LR: the probability-flow ODE of the reference's shift process (res_srdiff.py:7-25),
 * not the reference's stochastic step.  step_noise and x0 clipping are refused.  C*h*w must be a multiple of 4. */
typedef enum {
    MRISR_STEP_DDIM = 0, MRISR_STEP_RESSHIFT = 1, MRISR_STEP_DDPM = 2, MRISR_STEP_UNIPC = 3, MRISR_STEP_DPMSOLVERPP = 4
} mrisr_step_kind;
/* timesteps: host int64[n_steps]; alphas_cumprod: host f32[n_train]; unet required, controlnet may be NULL. */
int mrisr_sampler_create(mrisr_model* unet, mrisr_model* controlnet, int step_kind, const int64_t* timesteps,
                         int n_steps, const float* alphas_cumprod, int n_train, mrisr_sampler** out);
void mrisr_sampler_destroy(mrisr_sampler* s);
/* Runs all steps on `stream`, updating latents [B,C,h,w] f32 NCHW in place.
 *   lr_latents: RESSHIFT anchor (NULL for DDIM);  step_noise: RESSHIFT [n_steps-1 or more][B,C,h,w] f32 or NULL (then
 *   the stochastic term is dropped);  ehs / cond / intrablock as in the forward calls (projected once, before step 0).
 *   use_graph: capture step 0's launches into a hipGraph and replay it for the remaining steps. */
int mrisr_sampler_run(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                      const mrisr_tensor* step_noise, const mrisr_tensor* ehs, const mrisr_tensor* cond,
                      const mrisr_tensor* intrablock, int n_intrablock, int use_graph, void* stream);

/* Restrict the next runs to steps [first_step, last_step) of the schedule (default: all).  Step i always uses the
 * schedule's own (t_i, t_{i+1}) pair, so a truncated run reproduces the prefix of the full trajectory. */
int mrisr_sampler_set_range(mrisr_sampler* s, int first_step, int last_step);
/* DDPM only: clip the predicted x0 to [-range, range] (diffusers clip_sample / clip_sample_range); range <= 0 disables
 * (the default, as in the SD-1.5 scheduler config). */
int mrisr_sampler_set_clip(mrisr_sampler* s, float clip_sample_range);
/* Feature cache for the next runs (default: interval 1 = none; the step graph is then the one without it).  With interval N > 1,
 * step i of a run over [first_step, last_step) is a full forward that stores the cache when (i - first_step) % N == 0 and a shallow
 * forward that reads it otherwise (mrisr_unet_forward_cached), so the first step of every run is full and no run reads an earlier
 * run's cache.  The sampler owns the buffer (2B rows in a guided run) and keeps two step graphs.  depth: 1 .. num_skips-1.  Works
 * with every step kind, guidance, the LR anchor, step noise and adapter features; a sampler with a ControlNet refuses interval > 1.
 * The result deviates from the uncached run: the deep features of the last full step stand in for the current ones. */
int mrisr_sampler_set_cache(mrisr_sampler* s, int interval, int depth);
/* Multistep kinds only (defaults: order 2, final point "zero").  solver_order: 1..3 for UniPC, 1..2 for DPM-Solver++.
 * final_sigmas_zero: 1 - the last step lands on alpha = 1, sigma = 0 (diffusers' final_sigmas_type "zero"; that step is first order);
 * 0 - on alphas_cumprod[0] ("sigma_min", as the DDIM kind).  lower_order_final must be 1: UniPC's order is min(solver_order, steps
 * left, steps taken + 1); DPM-Solver++ drops to first order on the last step when n_steps < 15.  disable_corrector: UniPC step
 * indices without a corrector (NULL / 0: none).  A run restricted by mrisr_sampler_set_range starts COLD at first_step (order 1, no
 * corrector there: the history of the steps before it is not available), so for these kinds a split run differs from the full one. */
int mrisr_sampler_set_solver(mrisr_sampler* s, int solver_order, int final_sigmas_zero, int lower_order_final,
                             const int* disable_corrector, int n_disable);

/* ---- classifier-free guidance (off unless mrisr_sampler_run_guided is called) ----------------------
 * A guided step of B slices is ONE forward of 2B rows inside the same captured graph plus one fused step kernel.  Row order is
 * diffusers': rows 0..B-1 of ehs2 / cond2 / intrablock2 (and of the network's output) are the UNCONDITIONAL half, rows B..2B-1 the
 * CONDITIONAL half.  Per element, with g = guidance_scale and phi = guidance_rescale (Lin et al., "Common Diffusion Noise
 * Schedules and Sample Steps are Flawed", sec. 3.4):
 *     e = eps_u + g (eps_c - eps_u)
 *     phi > 0:  e = e (phi std_b(eps_c) / std_b(e) + (1 - phi))     std_b: over the C*h*w elements of sample b, unbiased (n-1)
 *                                                                    like torch.std; a sample with std_b(e) == 0 is left as it is
 *     x = the sampler's own DDIM / Res-SRDiff / DDPM update of x with e
 * latents, lr_latents and the step_noise slabs stay [B]: both halves share them.  g = 1 gives the conditional prediction, so
 * the defaults (g = 1, phi = 0) make a guided run a dearer form of the plain one.  The values are read by the next
 * mrisr_sampler_run_guided; plain mrisr_sampler_run ignores them.  phi must lie in [0, 1]. */
int mrisr_sampler_set_guidance(mrisr_sampler* s, float guidance_scale, float guidance_rescale);
/* As mrisr_sampler_run, with ehs2 [2B, L, D], cond2 [2B, 3, 8h, 8w] or NULL and every intrablock2 feature [2B, ...]; C*h*w of the
 * latents must be a multiple of 4.  ControlNet runs on both halves.  mrisr_sampler_set_range keeps its meaning. */
int mrisr_sampler_run_guided(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                             const mrisr_tensor* step_noise, const mrisr_tensor* ehs2, const mrisr_tensor* cond2,
                             const mrisr_tensor* intrablock2, int n_intrablock, int use_graph, void* stream);

/* ---- perturbed-attention guidance (PAG; Ahn et al. 2024, "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance") -----
 * Off unless mrisr_sampler_run_pag is called.  PAG needs no unconditional prompt: every step also predicts eps_p, the network's output
 * with the self-attention map of the applied blocks replaced by the identity (mrisr_model_set_pag: attn1 = to_out.0(to_v(norm1(h))), the
 * LoRA / DoRA terms of to_v and to_out.0 included; attn2, the feed-forward, the other blocks, ControlNet residuals and adapter features are
 * the conditional ones), and extrapolates away from it.  With s = pag_scale >= 0, g = guidance_scale, phi = guidance_rescale:
 *     PAG alone      (with_cfg == 0, forward of 2B rows [eps_p; eps_c]):         e = eps_c + s (eps_c - eps_p)
 *     PAG with CFG   (with_cfg != 0, forward of 3B rows [eps_p; eps_u; eps_c]):  e = eps_u + g (eps_c - eps_u) + s (eps_c - eps_p)
 *     phi > 0:  e = e (phi std_b(eps_c) / std_b(e) + (1 - phi))     exactly the rule of mrisr_sampler_set_guidance (unbiased, per sample,
 *                                                                    a sample with std_b(e) == 0 is left as it is)
 *     x = the sampler's own DDIM / Res-SRDiff / DDPM / UniPC / DPM-Solver++ update of x with e
 * Row order: PERTURBED rows first, CONDITIONAL rows last.  PAG alone is therefore the guided step with eps_0 := eps_p and g := 1 + s; the
 * unperturbed samples are one contiguous range (one attention launch per applied block); with tiles, sample b owns tile rows b T .. b T + T - 1
 * and the perturbed range is [0, B T).  Perturbed rows of ehsK carry the CONDITIONAL context; condK / intrablockK repeat the [B] operands K
 * times.  block_mask: bit i = transformer block i in forward order (mrisr_model_num_transformer_blocks).  g and phi are those of
 * mrisr_sampler_set_guidance (g is ignored by PAG alone).  s is a launch constant here; a per-step (adaptive) scale comes from
 * mrisr_sampler_set_schedule.  Refused before any launch:
 * s < 0 or not finite, s > 0 with an empty mask, a mask bit beyond the last block, a run with an empty mask, a feature cache with
 * interval > 1, a UNet built with fp8_attention, C*h*w of the latents not a multiple of 4.  During the run the UNet handle carries the pag
 * state of samples [0, B T); it is cleared when the call returns, also on an error.  The step graphs are keyed on (K, block_mask, s): a
 * change captures again, and mrisr_sampler_run / _run_guided keep their graphs' keys.  s == 0 is valid here and yields eps_c at the cost of
 * the larger forward; callers that want "off" call mrisr_sampler_run / _run_guided. */
int mrisr_sampler_set_pag(mrisr_sampler* s, uint32_t block_mask, float pag_scale);
/* As mrisr_sampler_run, with ehsK [K B, L, D], condK [K B, 3, 8h, 8w] or NULL and every intrablockK feature [K B, ...], K = 2 (with_cfg == 0)
 * or 3; tiled: K B T rows, sample-major.  ControlNet runs on all K B rows, unperturbed. */
int mrisr_sampler_run_pag(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents, const mrisr_tensor* step_noise,
                          const mrisr_tensor* ehsK, const mrisr_tensor* condK, const mrisr_tensor* intrablockK, int n_intrablock, int with_cfg,
                          int use_graph, void* stream);
/* step graphs this sampler has captured so far (a run whose key matches the previous one captures nothing) */
int mrisr_sampler_num_captures(const mrisr_sampler* s);

/* ---- skipping neutral steps ---------------------------------------------------------------------
 * Off by default.  With on != 0 each step of the following runs leaves out what its table rows (mrisr_sampler_set_schedule,
 * mrisr_sampler_set_conditioning; row i belongs to step i, also under mrisr_sampler_set_range) make neutral:
 *   - a guided / pag run whose schedule row has g == 1 and s == 0 (pag alone: s == 0; phi does not matter) forwards the B conditional rows
 *     only - the last B T of the K B T - and takes the reduced step, which writes the new state to every part of the staging buffer;
 *   - a conditioning row with c == 0 launches neither the ControlNet nor the residual adds;
 *   - a conditioning row with a == 0 hands the UNet no adapter features.
 * A run without the table has nothing to skip.  Each of the up to 8 step variants is its own graph, captured the first time a run needs it
 * from the one step plan (mrisr_sampler_num_captures counts each); other table values with the same neutral pattern replay them.  Refused
 * together with a feature cache (interval > 1), by either setter.  With on == 0: the launches, bits and captures of a sampler without it. */
int mrisr_sampler_set_skip(mrisr_sampler* s, int on);
/* the last run: out = {sum over its steps of the rows of the UNet forward, steps that ran the ControlNet, steps that took adapter features,
 * distinct step variants} */
int mrisr_sampler_run_stats(const mrisr_sampler* s, int64_t out[4]);

/* ---- FreeU (Si et al. 2023, "FreeU: Free Lunch in Diffusion U-Net"; the rule of diffusers' apply_freeu / fourier_filter) -----------
 * Off unless mrisr_model_set_freeu turned it on.  It rebalances the two inputs of the first two decoder blocks: the backbone half of the
 * hidden tensor is amplified by b, and the lowest spatial frequencies of the skip tensor - the one that already carries ControlNet
 * residuals and adapter features - are scaled by s.  Stage k is up block k in forward order (diffusers' resolution_idx rule, not the
 * original repository's channel-count rule).  FreeU v2's structure-aware backbone map is not implemented: b is a plain scalar.
 * fourier_filter, per (sample, channel) plane of H x W pixels: fftn, fftshift, the block [H/2-1 : H/2+1, W/2-1 : W/2+1] times s,
 * ifftshift, ifftn, real part.  The block holds the frequencies ky in {0, H-1}, kx in {0, W-1} as distinct residues (H == 1 or W == 1
 * leaves one on that axis; H == 2 leaves both), so with X the forward DFT
 *     y = x + (s - 1) / (H W) Re( sum over those <= 4 (ky, kx) of X(ky, kx) exp(+2 pi i (ky y / H + kx x / W)) )
 * which is what the kernel evaluates: sums in f32 (also for bf16 activations, as diffusers filters in f32), the result rounded once to the
 * activation dtype, no atomics - the bits repeat, and a graph replay equals the eager run.  One launch per decoder stage, six per
 * forward of a UNet with layers_per_block == 2.  Works with every step kind, classifier-free guidance, perturbed-attention guidance (the
 * perturbed rows are filtered like the others), tiles (per-tile planes), ControlNet residuals, adapter features, LoRA / DoRA and the
 * fp8 modes.  Not with the feature cache and not in a training step. */

/* ---- per-step schedule of the guidance and FreeU strengths --------------------------------------------------------------------------
 * Off unless mrisr_sampler_set_schedule set a table.  One f32 row of 8 per step of the sampler's schedule, row i for step i (an absolute
 * index, like the coefficient rows: mrisr_sampler_set_range keeps its meaning):
 *     { g, s, phi, freeu_s1, freeu_s2, freeu_b1, freeu_b2, 0 }       g = guidance_scale, s = pag_scale, phi = guidance_rescale
 * The neutral row {1, 0, 0, 1, 1, 1, 1, 0} makes the guided prediction the conditional one and FreeU the identity.  The sampler owns the
 * device table (reserved once, uploaded on the run's stream before the first step); the fused step kernels read g, s, phi from row
 * *step and the FreeU launches their two scalars, with ordinary loads behind the load of the step counter.  The values are NOT part of
 * the graph key: a run whose table has other values replays the stored graph.  Part of the key are the table's address and two flags:
 * "some row has phi > 0" (the rescale kernel runs for every step; a row with phi == 0 gets the factor exactly 1) and "FreeU reads the
 * table" (the UNet has FreeU on; its own four values are then not read).  The run kind is still decided by the entry point called -
 * plain, guided (K = 2), PAG alone (K = 2, the kernel forms g = 1 + s), PAG with CFG (K = 3) - and the scalars of
 * mrisr_sampler_set_guidance / _set_pag (the block mask apart) are not read while a table is set.  A neutral step costs a guided step.
 * rows_host NULL / n_rows 0 clears the table.  Refused before any device work, the message naming the field: n_rows != n_steps, a value
 * that is not finite, s < 0, phi outside [0, 1], a FreeU value < 0.  Refused by the run before any launch: FreeU columns other than 1
 * while the UNet has FreeU off; rows with s > 0 in a run that is not a PAG run; rows with g != 1 in a run with no unconditional half.
 * Everything the runs refuse without a table stays refused. */
int mrisr_sampler_set_schedule(mrisr_sampler* s, const float* rows_host, int n_rows);

/* ---- conditioning strength: ControlNet and adapter scale per step, guess mode ---------------------------------------------------------
 * Off unless mrisr_sampler_set_conditioning set a table: every ControlNet residual and adapter feature is then added at full strength,
 * with the launches and the bits of before.  One f32 row of 4 per step of the sampler's schedule, row i for step i (an absolute index,
 * like the coefficient rows and the schedule table above: mrisr_sampler_set_range keeps its meaning):
 *     { c, a, 0, 0 }       c = ControlNet conditioning scale of the step, a = adapter conditioning scale of the step
 * The neutral row is {1, 1, 0, 0}.  The sampler owns the device table (reserved once, one address for its life, uploaded on the run's
 * stream before the first step).  While a table is set the UNet adds the residuals with a multi-tensor scaled add,
 *     x_k = round_T( fma(f_k, r_k, x_k) )       f_k = w_k * c (residuals) or a (features), the product rounded once in f32,
 * one launch for the down residuals, one for the mid residual, one per adapter feature; the kernel reads c / a from row *step with ordinary
 * loads behind the load of the step counter, and reads r_k where the ControlNet's output convolutions wrote it.  The values are NOT part
 * of the graph key: a run whose table has other values replays the stored graph.  Part of the key: the table's address, guess mode, the
 * rows of the ControlNet's forward.  A step with c == 0 still runs the ControlNet.
 * guess_mode != 0 (diffusers' guess_mode): w_k = logspace(-1, 0, n_down + 1)[k], the mid residual last at weight 1 (otherwise w_k = 1).
 * In mrisr_sampler_run_guided the ControlNet then runs on the B conditional rows only - its input the last B rows of the staging buffer,
 * its context the last B rows of ehs2, cond2 given at [B] - and its residuals are added to rows [B, 2B) of the UNet's batch; the
 * unconditional rows get none.  In mrisr_sampler_run guess mode is the weights alone.
 * rows_host NULL / n_rows 0 clears the table (and guess mode).  Refused before any device work, the message naming row and field:
 * n_rows != n_steps, a value that is not finite, a non-zero column 2 or 3.  Refused by the run before any launch: rows with c != 1, or
 * guess mode, on a sampler without a ControlNet; rows with a != 1 in a run without adapter features; guess mode in a PAG run or with
 * tiles; a table together with a feature cache.  Everything the runs refuse without a table stays refused. */
int mrisr_sampler_set_conditioning(mrisr_sampler* s, const float* rows_host, int n_rows, int guess_mode);

/* ---- low-frequency consistency (ILVR: Choi et al., ICCV 2021) ------------------------------------
 * Off by default.  With a table, every step of the following runs ends with one more launch, after the reverse step and before the step
 * counter advances, on the latent canvas:
 *     x  <-  x + w phi_N( alpha ref + beta lr + sigma z - x )        {w, alpha, beta, sigma} = rows[step],   z = noise slab `step`
 * phi_N: the mean over each N x N block (N = factor, 2 .. 8, dividing h and w), upsampled by N back to [h, w] with `filter`:
 * MRISR_CONSIST_BILINEAR (torch's F.interpolate(F.avg_pool2d(d, N), scale_factor=N, mode="bilinear", align_corners=False): source
 * coordinate (i + 0.5) / N - 0.5, negative clamped to 0, upper neighbour clamped to the last cell) or MRISR_CONSIST_NEAREST (an exact
 * projection: at w = 1 the block means of the new x are those of the target).  ILVR itself filters bicubically both ways.
 * ref: f32 [B, C, h, w]; noise: f32 [n_steps, B, C, h, w] or NULL (slab i is read when row i has sigma != 0 - a table with such a row needs
 * it); lr: the run's lr_latents (NULL: no beta term).  Both pointers are REMEMBERED for the following runs: the caller keeps the buffers
 * alive.  The new x goes to the latents and, in a guided / pag run, to every part of the staging buffer (also on a reduced step).
 * The kernel reads its row with ordinary loads behind the load of the step counter, so the values are NOT part of the graph key: a run
 * whose table has other values replays the stored graph.  Part of the key: the table's address, factor, filter, the ref and noise
 * addresses.  A row with w == 0 still launches the kernel, which returns at once and leaves every bit as it was.
 * rows_host NULL / n_rows 0 clears everything (ref and noise are ignored).  Refused before any device work: n_rows != n_steps, a value
 * that is not finite, a factor or filter outside the accepted set, ref / noise that are not f32 of the shapes above (C: the UNet's
 * in_channels), a sigma != 0 without noise, a feature cache with interval > 1.  Refused by the run before any launch: latents of another
 * shape than ref, a factor that does not divide h and w of the canvas, a canvas that needs more than 64 KB of LDS,
 * 4 (h w / N + h w / N^2) bytes (128 x 128 latents at N = 2 need 48 KB; 256 x 256 needs N >= 8), a feature cache. */
typedef enum { MRISR_CONSIST_BILINEAR = 0, MRISR_CONSIST_NEAREST = 1 } mrisr_consist_filter;
int mrisr_sampler_set_consistency(mrisr_sampler* s, int factor, int filter, const float* rows_host, int n_rows, const mrisr_tensor* ref,
                                  const mrisr_tensor* noise);

/* ---- tiled sampling (MultiDiffusion, Bar-Tal et al. 2023, with the Gaussian weights of Mixture of Diffusers, Jimenez 2023) -------
 * The latent canvas [NB, C, H, W] is cut into overlapping tiles, the forward runs on the tile batch [NB*T, C, t_h, t_w] and the tile
 * predictions are blended back before the reverse step, which stays on the canvas.  All sizes in latent pixels.
 * Grid, per axis (extent n, tile t, overlap o, 0 <= o < t): t_eff = min(t, n); one tile at 0 if n <= t; else stride s = t - o,
 * k = ceil((n - t) / s) + 1 tiles, origin i = min(i s, n - t): the last tile is pulled back to end at n.  T = k_y k_x, tile index
 * ti = ty k_x + tx, row of the tile batch r = b T + ti (sample-major; b over the forward's rows: 2B in a guided run).
 * Window, per axis, length t_eff: uniform 1, or gaussian w[i] = exp(-((i - (t_eff-1)/2) / t_eff)^2 / (2 * 0.01)).  The normalised table
 * is nw[tile][i] = w[i] / (sum over the tiles covering origin + i of w[their local index]), float64 rounded once to f32; a pixel one
 * tile covers gets exactly 1.  Blend: eps[b,c,y,x] = sum over covering (ty, tx), ty then tx ascending, of
 * (nwy[ty][y - oy[ty]] * nwx[tx][x - ox[tx]]) * et[r, c, y - oy[ty], x - ox[tx]] - a gather per element, no atomics. */
typedef enum { MRISR_TILE_UNIFORM = 0, MRISR_TILE_GAUSSIAN = 1 } mrisr_tile_window;
/* One axis on the host (no GPU call): origins[n_tiles], weights[n_tiles][min(tile, extent)].  origins / weights may be NULL to ask
 * for n_tiles alone (never more than extent). */
int mrisr_tile_tables(int extent, int tile, int overlap, int window, int* origins, float* weights, int* n_tiles);
/* Tiles for the next runs; tile_h == 0 turns them off (the default).  tile and overlap must be multiples of d = 2^(num_levels-1),
 * tile >= d, 0 <= overlap < tile.  Refused while a feature cache is set (and mrisr_sampler_set_cache refuses interval > 1 while tiles
 * are set).  A run whose grid has T == 1 (tile >= canvas on both axes) is the plain run.  With T > 1, mrisr_sampler_run / _run_guided
 * take ehs [NB*T, L, D], cond [NB*T, 3, 8 t_h, 8 t_w] and intrablock features [NB*T, ...] at tile geometry (rows sample-major as
 * above); latents, lr_latents and step_noise stay canvas-shaped, and h, w of the canvas must be multiples of d. */
int mrisr_sampler_set_tiles(mrisr_sampler* s, int tile_h, int tile_w, int overlap_h, int overlap_w, int window);

/* ---- T2I-Adapter training (in BASELINE config 3 the adapter runs, and is differentiated, every step)
 * Same ownership model as the LoRA step: the caller owns ONE flat f32 vector of all adapter parameters (PyTorch layouts,
 * state-dict keys via tensor_info) and its gradient.  After train_prepare / train_bind, mrisr_adapter_forward keeps what the
 * backward needs; mrisr_adapter_backward takes the gradients w.r.t. the four feature maps (what mrisr_train_step wrote
 * through mrisr_train_set_intrablock_grads) and ADDS dW, db of every conv to the gradient vector (dgrad convs + one
 * pixel-contraction GEMM per conv).  refresh re-packs the kernels' weight layouts after the optimiser step. */
int mrisr_adapter_train_prepare(mrisr_adapter* a, void* stream);
int64_t mrisr_adapter_train_num_trainable(const mrisr_adapter* a);
int mrisr_adapter_train_num_tensors(const mrisr_adapter* a);
int mrisr_adapter_train_tensor_info(const mrisr_adapter* a, int i, const char** key, int64_t* offset, int64_t shape[4], int* ndim);
int mrisr_adapter_train_bind(mrisr_adapter* a, float* theta_dev, float* grad_dev, int init_from_model, void* stream);
int mrisr_adapter_train_refresh(mrisr_adapter* a, void* stream);
int mrisr_adapter_backward(mrisr_adapter* a, const mrisr_tensor* d_feats, int n_feats, void* stream);
/* The same pass cut at level boundaries, so that the host can start the exchange of a level's finished weight gradients while
 * the lower levels are still being differentiated: call with level = top level, ..., 0 (level 0 also
 * differentiates conv_in).  mrisr_adapter_train_level_range: that level's contiguous range of the flat trainable vector. */
int mrisr_adapter_backward_level(mrisr_adapter* a, const mrisr_tensor* d_feats, int n_feats, int level, void* stream);
int mrisr_adapter_train_level_range(const mrisr_adapter* a, int level, int64_t* offset, int64_t* numel);

/* ---- AutoencoderKL (SD-1.5 VAE): pixel <-> latent, once before / once after the sampling loop --------------
 * Replaces vae.encode(x).latent_dist (res_srdiff.py:49-50) and vae.decode(z).sample (res_srdiff.py:107-110); the
 * arithmetic is diffusers' AutoencoderKL (state-dict keys encoder.* / decoder.* / quant_conv / post_quant_conv).
 *   encode: image [B,3,H,W] -> moments [B, 2*latent, H/8, W/8] = (mean | logvar) of the diagonal Gaussian posterior;
 *           sampling (mean + exp(0.5*logvar)*eps) and the scaling_factor stay with the caller, as in the reference.
 *   decode: latents [B,latent,h,w] (already divided by scaling_factor) -> image [B,3,8h,8w], NCHW in image->dtype. */
typedef struct {
    int32_t in_channels;           /* 3 */
    int32_t out_channels;          /* 3 */
    int32_t latent_channels;       /* 4 */
    int32_t num_levels;            /* 4 */
    int32_t block_out_channels[4]; /* 128, 256, 512, 512 */
    int32_t layers_per_block;      /* 2 */
    int32_t norm_num_groups;       /* 32 */
    int32_t compute_dtype;         /* MRISR_BF16 or MRISR_F32 */
    float scaling_factor;          /* 0.18215 (carried for the host mirror; not applied by encode / decode) */
} mrisr_vae_cfg;
typedef struct mrisr_vae mrisr_vae;
int mrisr_vae_create(const mrisr_vae_cfg* cfg, mrisr_vae** out);
void mrisr_vae_destroy(mrisr_vae* v);
int mrisr_vae_set_param(mrisr_vae* v, const char* key, const float* data, const int64_t* shape, int ndim, int is_device);
int64_t mrisr_vae_num_params(const mrisr_vae* v);
int mrisr_vae_finalize(mrisr_vae* v, void* stream);
int mrisr_vae_encode(mrisr_vae* v, const mrisr_tensor* image, mrisr_tensor* moments, void* stream);
int mrisr_vae_decode(mrisr_vae* v, const mrisr_tensor* latents, mrisr_tensor* image, void* stream);

/* ---- LoRA fine-tuning step ---------------------------------------------------
 * Replaces, for the UNet handle, what the reference's training cell gets from torch autograd + accelerate
 * (notebook ResDif c11:14-41: noise_pred = unet(noisy, t, ehs).sample; loss = mse(noise_pred, noise);
 *  accelerator.backward(loss); clip_grad_norm_(1.0); optimizer.step()).  Base weights are frozen; the trainable
 * parameters are the peft adapters (<module>.lora_A/B.default.weight), kept by the CALLER as ONE flat f32 device
 * vector `theta` with a gradient vector `grad` of the same length - the bucket a data-parallel host all-reduces.
 *   prepare      - packs the transposed / tap-flipped weight copies the dX GEMMs read and lays out theta
 *   tensor_info  - i-th adapter tensor: state-dict key, element offset in theta, shape {rows, cols}
 *   bind         - attaches theta / grad (init_from_model: theta <- the adapters loaded with set_param)
 *   step         - forward, loss = mean((eps_hat - target)^2) -> *loss_dev, backward; adapter gradients are ADDED to
 *                  grad (zero it per optimiser step; accumulating several micro-batches is allowed).  target: f32
 *                  NCHW.  pred_out (optional): eps_hat.  The model must be created with lora_fused = 1.
 *   refresh      - re-packs the adapters from theta after the optimiser changed it
 *   optim_sumsq  - *out_dev += sum(g^2)   (global grad norm; all-reduce it with the gradients)
 *   optim_adamw  - torch.optim.AdamW update on flat vectors; g is first scaled by grad_scale (1/world_size after a
 *                  sum all-reduce) and, when max_norm > 0, by min(1, max_norm / (grad_scale*sqrt(*sumsq_dev) + 1e-6))
 *                  as torch.nn.utils.clip_grad_norm_ does; step counts from 1. */
int mrisr_train_prepare(mrisr_model* m, void* stream);
int64_t mrisr_train_num_trainable(const mrisr_model* m);
int mrisr_train_num_tensors(const mrisr_model* m);
int mrisr_train_tensor_info(const mrisr_model* m, int i, const char** key, int64_t* offset, int64_t shape[2]);
/* The PyTorch shape of trainable tensor i: 4-D ([r, cin, 3, 3] / [cout, r, 1, 1]) for the adapters of a resnet's 3x3 convs, 2-D for the
 * rest.  (mrisr_train_tensor_info reports a conv tensor as rows = shape[0], cols = the product of the others.) */
int mrisr_train_tensor_shape(const mrisr_model* m, int i, int64_t shape[4], int* ndim);
int mrisr_train_bind(mrisr_model* m, float* theta_dev, float* grad_dev, int init_from_model, void* stream);
int mrisr_train_refresh(mrisr_model* m, void* stream);
int mrisr_train_step(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                     const mrisr_tensor* intrablock, int n_intrablock, const mrisr_tensor* target, float* loss_dev,
                     mrisr_tensor* pred_out, void* stream);
/* Gradients w.r.t. the T2I-Adapter features (intrablock[i] of the following mrisr_train_step calls) are written to
 * grads[i] (same shapes; NCHW f32/bf16 or NHWC compute dtype) for the adapter's own backward; n = 0 switches it off. */
int mrisr_train_set_intrablock_grads(mrisr_model* m, const mrisr_tensor* grads, int n);
/* ControlNet residuals for the following mrisr_train_step calls (reference call shape: unet(..., down_block_additional_residuals=down_res,
 * mid_block_additional_residual=mid_res), src/adapters/res_srdiff.py:73-78, inside the training graph): down[k] / mid are added to the skips /
 * the mid block's output (out of place, as diffusers does), and d(loss)/d(down[k]), d(loss)/d(mid) are written to d_down[k] / d_mid (same
 * shapes; may be null) - the seeds of the ControlNet's own backward (mrisr_controlnet_train_step).  n_down = 0, mid = NULL switches it off.
 * The UNet may be frozen (lora_rank 0: mrisr_train_bind(m, NULL, NULL, 0, stream)): the step then only computes these input gradients. */
int mrisr_train_set_controlnet_residuals(mrisr_model* m, const mrisr_tensor* down, const mrisr_tensor* d_down, int n_down,
                                         const mrisr_tensor* mid, const mrisr_tensor* d_mid);
/* ---- ControlNet with its own parameters trainable (NOT in the reference's code: it only runs a ControlNet for inference,
 * src/adapters/res_srdiff.py:65-70; SURVEY.md 3.2 lists it as a training configuration).  The ControlNet handle's raw tensors live in
 * ONE flat f32 vector the caller owns (offsets by mrisr_controlnet_train_tensor_info, key order = sorted state-dict names); one training
 * step is  train_forward (recorded; writes the 12 + 1 residuals) -> mrisr_train_step of the UNet with those residuals
 * (mrisr_train_set_controlnet_residuals: it writes d(loss)/d(residual)) -> train_backward (adds d(loss)/d(parameter) to the gradient
 * vector) -> all-reduce, mrisr_optim_adamw on the flat vectors -> train_refresh (re-packs every weight in place).
 * `differentiated` = 0 marks tensors whose gradient this build leaves at zero (norm affine parameters, the time-embedding MLP and its
 * per-block projections, the condition embedding): keep them out of the optimiser or accept that they stay frozen. */
int mrisr_controlnet_train_prepare(mrisr_model* m, void* stream);
int64_t mrisr_controlnet_train_num_trainable(const mrisr_model* m);
int mrisr_controlnet_train_num_tensors(const mrisr_model* m);
int mrisr_controlnet_train_tensor_info(const mrisr_model* m, int i, const char** key, int64_t* offset, int64_t* numel, int* differentiated);
int mrisr_controlnet_train_bind(mrisr_model* m, float* theta_dev, float* grad_dev, int init_from_model, void* stream);
int mrisr_controlnet_train_refresh(mrisr_model* m, void* stream);
int mrisr_controlnet_train_forward(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                                   const mrisr_tensor* cond, float conditioning_scale, mrisr_tensor* down_out, int n_down, mrisr_tensor* mid_out,
                                   void* stream);
int mrisr_controlnet_train_backward(mrisr_model* m, const mrisr_tensor* d_down, int n_down, const mrisr_tensor* d_mid, float conditioning_scale,
                                    void* stream);
int mrisr_optim_sumsq(const float* g_dev, int64_t n, float* out_dev, void* stream);
/* ema = decay * ema + (1 - decay) * theta  (diffusers EMAModel.step on the flat trainable vector) */
int mrisr_optim_ema(float* ema_dev, const float* theta_dev, int64_t n, float decay, void* stream);
int mrisr_optim_adamw(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, const float* sumsq_dev,
                      float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                      int step, void* stream);

/* ---- fine-tuning loop on the device (mrisr.fit; notebook ResDif c11:14-41) -------------------------------------------------
 * One optimiser step = `accum` launches of mrisr_fit_micro (graph M) + one mrisr_fit_apply (graph O); with world > 1 the caller
 * all-reduces the bound grad vector between them.  Both graphs read the optimiser step s and micro-batch k from a device counter.
 *   micro      - batch builder -> mrisr_train_step (adds into grad) -> loss accumulated, k + 1.  Re-captured whenever the UNet's
 *                workspace was re-planned (a validation forward, another geometry) - planning itself never runs inside a capture.
 *   apply      - sumsq -> AdamW with lr / bias correction from the step's table row, grad_scale = 1 / (world * accum) -> adapter
 *                re-pack -> EMA with the step's decay (use_ema) -> rings[s] = {mean loss of the micro-batches, grad norm, lr} ->
 *                s + 1, k = 0 -> grad = 0
 *   make_batch - the batch builder alone for a given (s, k), eagerly, into caller buffers: sample / target [batch][C][h][w] f32,
 *                timesteps [batch] int64, ehs [batch][ctx_len][ctx_dim] f32; optional: eps_hr / eps_lr (the posterior-sampling noise,
 *                latent-shaped) and caption_row [batch] int32
 *   set_step   - counter <- {step, 0} (resume)
 * Batch builder, for sample b of micro-batch k of step s: item = index_table[(s * accum + k) * batch + b];
 *   z_hr = (mean_hr + std_hr * e_hr) * scaling_factor, z_lr likewise; t uniform on [0, num_train_timesteps); eps ~ N(0, 1);
 *   sample = sqrt(abar_t) z_hr + (1 - sqrt(abar_t)) z_lr + sqrt(1 - abar_t) eps, target = eps;
 *   ehs[b] = captions[caption_of_item[item]], or captions[empty_row] with probability proportion_empty.
 * Every random number is Philox4x32-10 keyed by (seed, s, k, sample_base + b, element, stream): the same (seed, s, k) gives the same
 * batch bit for bit, eager or captured, before or after a resume.
 * moments_dev: f32 [n_items][4][latent_channels * h * w] = {HR mean, HR std, LR mean, LR std}; captions_dev: f32
 * [n_captions][ctx_len][ctx_dim] (both caller-owned, alive as long as the handle).  Host tables, copied: caption_of_item [n_items],
 * index_table [max_steps * accum * batch], alphas_cumprod [num_train_timesteps], lr_table / ema_decay_table [max_steps] (value of
 * optimiser step s, s from 0).  The UNet must carry bound adapters (mrisr_train_bind); exp_avg / exp_avg_sq / ema are flat vectors of
 * its trainable length, the rings f32 [max_steps]. */
typedef struct mrisr_fit mrisr_fit;
typedef struct {
    int32_t batch, accum, max_steps, world;
    int32_t sample_base;            /* global index of this rank's first sample (rank * batch): keys the RNG */
    int32_t n_items, latent_channels, latent_h, latent_w;
    int32_t n_captions, ctx_len, ctx_dim;
    int32_t empty_row;              /* caption row of the empty prompt, -1: none */
    int32_t num_train_timesteps;
    int32_t use_ema;
    float proportion_empty, scaling_factor;
    float beta1, beta2, eps, weight_decay, max_grad_norm;
    uint64_t seed;
} mrisr_fit_config;
int mrisr_fit_create(mrisr_model* unet, const mrisr_fit_config* cfg, const float* moments_dev, const float* captions_dev,
                     const int32_t* caption_of_item, const int32_t* index_table, const float* alphas_cumprod, const float* lr_table,
                     const float* ema_decay_table, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, float* loss_ring_dev,
                     float* grad_norm_ring_dev, float* lr_ring_dev, mrisr_fit** out);
void mrisr_fit_destroy(mrisr_fit* f);
int mrisr_fit_set_step(mrisr_fit* f, int step, void* stream);
int mrisr_fit_get_step(const mrisr_fit* f);
int mrisr_fit_num_captures(const mrisr_fit* f);  /* graphs captured so far (M and O together) */
int mrisr_fit_micro(mrisr_fit* f, void* stream);
int mrisr_fit_apply(mrisr_fit* f, void* stream);
int mrisr_fit_make_batch(mrisr_fit* f, int step, int micro, float* sample_dev, int64_t* timesteps_dev, float* ehs_dev, float* target_dev,
                         float* eps_hr_dev, float* eps_lr_dev, int32_t* caption_row_dev, void* stream);
/* T2I-Adapter in the loop (the notebook's lora_rank: null run, or LoRA + adapter as joint_step trains them).  The UNet may be frozen
 * (n_trainable == 0).  Per micro-batch graph M then also builds the condition, runs the adapter forward, feeds its features to the UNet
 * step as intrablock residuals and their gradients to the adapter backward (adds into the adapter's bound grad); graph O clips BOTH
 * buckets by their joint norm (one sumsq, the grad-norm ring holds it), AdamW on each from the same lr table, adapter re-pack, EMA of
 * each (use_ema), zeroes both gradients.
 *   adapter          - train-prepared and bound (mrisr_adapter_train_bind), compute dtype of the UNet, cin 192, one feature per UNet
 *                      level with that level's channels
 *   cond_dev         - f32 [n_items][res][res]: each item's LR image (1 channel, in [-1, 1], at the training resolution), caller-owned
 *   res              - multiple of 8, res / 8 == latent_h == latent_w
 *   exp_avg / exp_avg_sq / ema - flat f32 vectors of the adapter's trainable length (ema: with use_ema)
 * make_condition - the condition of sample b of (step, micro) for the item make_batch draws, eagerly:
 *   form 0: f32 [batch][3][res][res] (the image expanded to 3 channels: the input of mrisr_adapter_forward);
 *   form 1: the adapter's input activation graph M uses, [batch][res/8][res/8][192] in the compute dtype, channel
 *           c * 64 + dy * 8 + dx = image[8 i + dy][8 j + dx] (PixelUnshuffle(8) of form 0, NHWC). */
typedef struct {
    mrisr_adapter* adapter;
    const float* cond_dev;
    int32_t res;
    float* exp_avg_dev;
    float* exp_avg_sq_dev;
    float* ema_dev;
} mrisr_fit_adapter_args;
int mrisr_fit_create_adapter(mrisr_model* unet, const mrisr_fit_config* cfg, const float* moments_dev, const float* captions_dev,
                             const int32_t* caption_of_item, const int32_t* index_table, const float* alphas_cumprod,
                             const float* lr_table, const float* ema_decay_table, float* exp_avg_dev, float* exp_avg_sq_dev,
                             float* ema_dev, float* loss_ring_dev, float* grad_norm_ring_dev, float* lr_ring_dev,
                             const mrisr_fit_adapter_args* adapter, mrisr_fit** out);
int mrisr_fit_make_condition(mrisr_fit* f, int step, int micro, void* out_dev, int form, void* stream);

/* ---- image metrics of the reference's evaluator (src/eval/eval.py:15-51) --------------------------------------
 * pred / gt: f32 [batch][height][width] in [0, 1] (the reference divides its 8-bit PNGs by 255).  out: f32 [batch][4] =
 * {PSNR (torchmetrics, data_range 1), SSIM (torchmetrics defaults: 11x11 Gaussian sigma 1.5, k1 .01, k2 .03, mean over
 * the fully-inside windows), HFEN (||LoG(pred) - LoG(gt)|| / (||LoG(gt)|| + 1e-8), sigma 1.5), NMSE}.
 * scratch: 2*batch*height*width floats; sums: batch*6 doubles (zeroed here). */
int mrisr_image_metrics(const float* pred_dev, const float* gt_dev, int batch, int height, int width, float* scratch_dev,
                        double* sums_dev, float* out_dev, void* stream);

/* ---- slice degradation of the reference's data pipeline (nb ResDif c22:102-154) ----------------
 * All images are f32 [batch][height][width] on the device.  scratch sizes come from the *_scratch_bytes functions.
 *   resize_slices:        Pillow Image.resize on mode "F" (filter 0 = BICUBIC a=-0.5, 1 = LANCZOS a=3; antialiased support when
 *                         shrinking) - replaces FastMRILazyDataset._pad_to_target's resize            nb ResDif c22:102-113
 *   gaussian_blur_slices: scipy.ndimage.gaussian_filter(sigma, mode "reflect", truncate)               nb ResDif c22:143-144
 *   simulate_low_field:   blur(sigma 0.5*scale) -> BICUBIC to the small size -> BICUBIC back            nb ResDif c22:140-154
 *                         (small size = (W//scale) rows x (H//scale) columns, the reference's own tuple order) */
size_t mrisr_resize_scratch_bytes(int batch, int height, int width, int out_height, int out_width, int filter);
int mrisr_resize_slices(const float* in_dev, int batch, int height, int width, float* out_dev, int out_height, int out_width, int filter,
                        void* scratch_dev, size_t scratch_bytes, void* stream);
int mrisr_gaussian_blur_slices(const float* in_dev, int batch, int height, int width, float sigma, float truncate, float* tmp_dev,
                               float* out_dev, void* stream);
size_t mrisr_low_field_scratch_bytes(int batch, int height, int width, float scale_factor);
int mrisr_simulate_low_field(const float* hr_dev, int batch, int height, int width, float scale_factor, float* lr_dev, void* scratch_dev,
                             size_t scratch_bytes, void* stream);

/* ---- per-launch HIP-event profiler (bench.py roofline leg; off by default) ------------------------- */
int mrisr_prof_enable(int on);
int mrisr_prof_reset(void);
/* JSON {"<kernel class>": {"launches", "ms", "flops", "bytes"}}; returns the length written or -1 if buf is too small */
int mrisr_prof_report(char* buf, int cap);

/* ---- single-op entry points (used by the parity tests; same kernels the models launch) ------------ */
int mrisr_op_conv3x3(const mrisr_tensor* x_nhwc, const mrisr_tensor* x2_nhwc, const float* w_oihw_dev,
                     const float* bias_dev, int cout, int stride, int upsample, int act, int splitk, int tile,
                     mrisr_tensor* y_nhwc, void* stream);
/* a resnet's conv2 with its 1x1 conv_shortcut (bf16, stride 1, channel counts multiples of 64): y = conv3x3([x | x2]) + bias +
 * W_sc [xs | xs2] + bias_sc, the shortcut sources read at the output pixel.  fused = 1: one launch, the shortcut as the last K steps of
 * the conv on a concatenated filter bank; fused = 0: the shortcut GEMM, then the conv with its output as the residual */
int mrisr_op_conv3x3_sc(const mrisr_tensor* x_nhwc, const mrisr_tensor* x2_nhwc, const float* w_oihw_dev, const float* bias_dev,
                        const mrisr_tensor* xs_nhwc, const mrisr_tensor* xs2_nhwc, const float* w_sc_dev, const float* bias_sc_dev,
                        int cout, int splitk, int tile, int fused, mrisr_tensor* y_nhwc, void* stream);
/* a transformer block's ff.net.2 followed by the transformer's proj_out (bf16 rows; widths multiples of 64):
 * y = (h W2^T + b2 + t) Wp^T + bp + x with h [M][K4], t / x / y [M][C], W2 [C][K4], Wp [C][C] (f32 on the device; biases may be NULL).
 * fused = 1: one launch over K = [K4 | C] on the composed weight [Wp W2 | Wp]; fused = 0: the two launches */
int mrisr_op_ff_proj(const mrisr_tensor* h_rows, const mrisr_tensor* t_rows, const mrisr_tensor* x_rows, const float* w2_dev,
                     const float* b2_dev, const float* wp_dev, const float* bp_dev, int tile, int fused, mrisr_tensor* y_rows, void* stream);
int mrisr_op_linear(const mrisr_tensor* x_rows, const float* w_dev, const float* bias_dev, int n, int act,
                    int splitk, int tile, mrisr_tensor* y_rows, void* stream);
/* a projection with everything its epilogue carries in the models (bf16 rows): y = x W^T + bias + rowvec[m / (M / rowvec_rows)] +
 * lora_scale B (A x) + resid.  rowvec f32 [rowvec_rows][n] (rowvec_rows divides M; 1 = one row for every output row), A [lora_r][K],
 * B [n][lora_r] f32 (lora_r = 0: no adapter, both NULL; an adapter takes no split-K); bias, rowvec and resid may be NULL; resid
 * [M][>= n] may be y itself (in place) */
int mrisr_op_linear_resid(const mrisr_tensor* x_rows, const float* w_dev, const float* bias_dev, int n, const float* rowvec_dev,
                          int rowvec_rows, const float* lora_a_dev, const float* lora_b_dev, int lora_r, float lora_scale,
                          const mrisr_tensor* resid_rows, int splitk, int tile, mrisr_tensor* y_rows, void* stream);
/* y = LayerNorm(x; gamma, beta, eps 1e-5) W^T + bias with the normalisation as a prologue of the row-panel GEMM kernel (bf16;
 * K = 320 or 640, n % 16 == 0) - the form the transformer blocks use for norm1/2/3 -> to_q|k|v / to_q / ff.net.0.proj */
int mrisr_op_ln_linear(const mrisr_tensor* x_rows, const float* gamma_dev, const float* beta_dev, const float* w_dev,
                       const float* bias_dev, int n, int act, mrisr_tensor* y_rows, void* stream);
/* y = [x +] FF2(GEGLU(FF1(LayerNorm(x)))) - the feed-forward of BasicTransformerBlock (diffusers attention.py: norm3 -> ff -> + hidden)
 * in ONE kernel at C = 320 (bf16): w1 = ff.net.0.proj.weight [2*hidden][320], w2 = ff.net.2.weight [320][hidden], f32 on the device */
int mrisr_op_mlp(const mrisr_tensor* x_rows, const float* gamma_dev, const float* beta_dev, const float* w1_dev, const float* b1_dev,
                 const float* w2_dev, const float* b2_dev, int hidden, int residual, mrisr_tensor* y_rows, void* stream);
/* the same kernel with its continuation, the transformer's proj_out and outer residual (MlpArgs::wp / bp / xres / out2):
 * y = ([x +] FF2(GEGLU(FF1(LayerNorm(x))))) Wp^T + bp + xres, wp = proj_out.weight [320][320] f32 (bp may be NULL), xres / y bf16 [M][320];
 * the feed-forward output itself is not returned.  M must be a multiple of 128 (whole row panels), else the call is refused */
int mrisr_op_mlp_proj(const mrisr_tensor* x_rows, const float* gamma_dev, const float* beta_dev, const float* w1_dev, const float* b1_dev,
                      const float* w2_dev, const float* b2_dev, int hidden, int residual, const float* wp_dev, const float* bp_dev,
                      const mrisr_tensor* xres_rows, mrisr_tensor* y_rows, void* stream);
/* the row-local middle of BasicTransformerBlock at C = 320, 8 heads, in ONE kernel (csrc/xtail.hip), in place on t:
 *   x1 = attn1.to_out(ao) + t;  q = attn2.to_q(LayerNorm2(x1));  o = softmax(q K^T / sqrt(40)) V per head;  t <- attn2.to_out(o) + x1
 * ao [M][ldao], t [M][ldt] bf16 (the tensors' second extent is the row pitch: >= 320, a multiple of 8; columns >= 320 are neither read nor
 * written); ntok tokens per image (a multiple of 128 dividing M); w1 / wq / w2 [320][320], gamma / beta [320] f32 on the device, biases
 * may be NULL; k, v the already projected prompt rows, bf16 [M / ntok][>= nk][320], of which the first nk (1 .. 80) are keys.  lora_r = 4:
 * a rank-4 adapter (A [4][320], B [320][4], f32) on each of the three projections, all scaled by lora_scale; lora_r = 0: all six NULL.
 * Weights, K / V and adapters are packed as the models pack them, on buffers of the call; anything the kernel is not written for is
 * refused before the first launch */
int mrisr_op_xattn_tail(const mrisr_tensor* ao_rows, mrisr_tensor* t_rows, int ntok, const float* w1_dev, const float* b1_dev,
                        const float* gamma_dev, const float* beta_dev, const float* wq_dev, const float* bq_dev, const float* w2_dev,
                        const float* b2_dev, const mrisr_tensor* k, const mrisr_tensor* v, int nk, const float* a1_dev, const float* lb1_dev,
                        const float* aq_dev, const float* lbq_dev, const float* a2_dev, const float* lb2_dev, int lora_r, float lora_scale,
                        void* stream);
/* the fp8 form of the same projection (BASELINE configs[4]): weights quantised to OCP e4m3 with one scale per output channel, the
 * rows with one scale per row inside the kernel, f32 accumulate; gamma_dev / beta_dev NULL = no LayerNorm prologue */
int mrisr_op_linear_fp8(const mrisr_tensor* x_rows, const float* gamma_dev, const float* beta_dev, const float* w_dev,
                        const float* bias_dev, int n, int act, mrisr_tensor* y_rows, void* stream);
int mrisr_op_groupnorm(const mrisr_tensor* x_nhwc, const mrisr_tensor* x2_nhwc, const float* gamma_dev,
                       const float* beta_dev, int groups, float eps, int silu, mrisr_tensor* y_nhwc, void* stream);
int mrisr_op_layernorm(const mrisr_tensor* x_rows, const float* gamma_dev, const float* beta_dev, float eps,
                       mrisr_tensor* y_rows, void* stream);
/* q,k,v rows [B,N,H*d] (k,v: [B,Nk,H*d]) -> out [B,N,H*d]; flash=1 uses the fused kernel (bf16) */
int mrisr_op_attention(const mrisr_tensor* q, const mrisr_tensor* k, const mrisr_tensor* v, int heads, int flash,
                       mrisr_tensor* out, void* stream);

/* gradients of mrisr_op_attention (bf16, flash path): dq [B,N,H*d], dk, dv [B,Nk,H*d] for an upstream dout [B,N,H*d] */
int mrisr_op_attention_bwd(const mrisr_tensor* q, const mrisr_tensor* k, const mrisr_tensor* v, const mrisr_tensor* dout,
                           int heads, mrisr_tensor* dq, mrisr_tensor* dk, mrisr_tensor* dv, void* stream);

/* ---- single-op entry points of the backward (csrc/bwd.hip, csrc/train_ops.h): each runs the launcher the training step runs, on
 * device pointers of the caller; `dtype` is MRISR_F32 or MRISR_BF16 (the type of every operand called T below), gradients of
 * parameters are f32 and are ADDED to what the output holds.  Every call checks the shapes and alignments its kernels assume before
 * the first launch and synchronises the stream before it returns. ---- */
/* GroupNorm(+SiLU) backward over x = [x0 | x1] (NHWC, T, [B][HW][c0] and [B][HW][c1]; x1 NULL with c1 = 0): the forward statistics
 * as the recorded forward computes them, then dx0 / dx1 (T; acc0 / acc1: add into them); g_gamma / g_beta [c0] (both or neither,
 * only without x1): the affine gradients.  Honours mrisr_debug_gn_fused (one-pass kernel or the two-kernel path). */
int mrisr_op_groupnorm_bwd(int dtype, const void* x0, int c0, const void* x1, int c1, int B, int HW, const float* gamma_dev,
                           const float* beta_dev, int groups, float eps, int silu, const void* dy, void* dx0, int acc0, void* dx1,
                           int acc1, float* g_gamma, float* g_beta, void* stream);
/* LayerNorm backward on rows [M][C] (T); g_gamma / g_beta [C] optional (both or neither); dx NULL: the affine gradients alone */
int mrisr_op_layernorm_bwd(int dtype, const void* x, const void* dy, void* dx, const float* gamma_dev, int M, int C, float eps,
                           int accumulate, float* g_gamma, float* g_beta, void* stream);
/* GEGLU on a stored pre-activation [M][2*half] in the projection's 16-wide (value, gate) interleave.  backward = 0: out [M][half] =
 * u * gelu(g) (dout unused); backward = 1: out [M][2*half] = d pre for an upstream dout [M][half] */
int mrisr_op_geglu(int dtype, int backward, const void* pre, const void* dout, void* out, int64_t M, int half, void* stream);
/* the element-wise / reduction group.  kind:
 *   0 silu_bwd     out[i] = a[i] * silu'(b[i])                      (a = dy, b = pre-activation; n elements)
 *   1 relu_bwd     out[i] = b[i] > 0 ? a[i] : 0                     (a = dy, b = the ReLU's output; n elements)
 *   2 sumpool2     out[B][H][W][C] (+)= 2x2 sums of a[B][2H][2W][C] (flag: accumulate)
 *   3 mse_grad     a = prediction NHWC T [B][H][W][C], b = target NCHW f32; out = d pred (T), out_f32[0] = the loss
 *   4 rowvec_grad  out_f32[(flag ? 0 : b) * ld_out + off + c] += sum_hw a[b][hw][c]   (a: [B][H*W][C]; flag: scalar timestep)
 *   5 colsum       out_f32[c] += sum_m a[m][c]                      (a: [B*H*W][C]) */
int mrisr_op_pointwise_bwd(int kind, int dtype, const void* a, const void* b, void* out, float* out_f32, int64_t n, int B, int H, int W,
                           int C, int flag, int ld_out, int off, void* stream);
/* LoRA weight gradients.  mode 0 (dB): out_j[secN][r] += scale * P_j^T Q_j, P = dY [M][C = nmod*secN] (T, pitch ldp), Q = z [M][nmod*r]
 * (f32, pitch ldq); mode 1 (dA): out_j[r][C] += scale * Q_j^T P, P = x [M][C].  r in {4, 8, 12, 16}, nmod <= 3; a NULL out_j is skipped */
int mrisr_op_lora_wgrad(int dtype, const void* P, int ldp, const float* Q, int ldq, int M, int C, int mode, int r, int nmod, int secN,
                        float* out0, float* out1, float* out2, float scale, void* stream);
/* dB of an adapter on ff.net.0.proj: P = d pre [M][2*half] (T, pitch ldp) in the projection's 16-wide (value, gate) interleave, Q = z [M][r]
 * (f32, pitch ldq); out [2*half][r] += scale * P^T Q with its rows in the raw order of lora_B (value rows [0, half), gate rows [half, 2*half)):
 * the un-interleave happens in the scatter of the reduction */
int mrisr_op_lora_wgrad_geglu(int dtype, const void* P, int ldp, const float* Q, int ldq, int M, int half, int r, float* out, float scale,
                              void* stream);
/* The same sums at rank r in {32, 48, ..., 128}.  Q is of type T, with module j's r columns at j * rp where rp is r rounded up to the K tile
 * of the engine (64 elements in bf16, 32 in f32); the columns past r are padding and are never read out.  ldq >= nmod * rp.  geglu_half > 0
 * (mode 0, nmod 1, C = 2 * geglu_half): P's columns are in the interleave of ff.net.0.proj and out0's rows in raw order, as above.
 * bf16 runs on the MFMA pipe (lora_wgrad_hr_kernel), f32 walks the streaming kernel over 16 columns of Q at a time */
int mrisr_op_lora_wgrad_hr(int dtype, const void* P, int ldp, const void* Q, int ldq, int M, int C, int mode, int r, int nmod, int secN,
                           float* out0, float* out1, float* out2, float scale, int geglu_half, void* stream);
/* DoRA.  W [n][k], A [r][k], B [n][r], mag [n]: f32 in PyTorch's row order.  g[dst(j)] = mag[j] / ||W[j,:] + scale (B A)[j,:]||_2 (f32), and row
 * dst(j) of out (T, pitch ld >= k) = g W[j,:] - or, merged != 0, g (W + scale B A)[j,:] - rounded once from the f32 product.  dst(j) = j, or
 * with geglu_half > 0 (n = 2 * geglu_half) the 16-wide (value, gate) interleave of ff.net.0.proj.  r: 4 / 8 / 12 / 16 or 32 .. 128 in steps of 16 */
int mrisr_op_dora_scale(int dtype, const float* W, const float* A, const float* B, const float* mag, float scale, float* g, void* out, int ld,
                        int n, int k, int r, int geglu_half, int merged, void* stream);
/* gm[c] += ( sum_m P[m][src(c)] (Y[m][src(c)] - R[m][src(c)]) - bias[src(c)] sum_m P[m][src(c)] ) / mag[c]: the gradient of a DoRA magnitude from
 * P = dY and the projection's output Y (less the residual R its epilogue added, less its bias).  P, Y, R: T, row-major [M][C] with pitches ldp,
 * ldy, ldr >= C; R and bias may be NULL; C a multiple of 8.  src(c) = c, or with geglu_half > 0 (C = 2 * geglu_half) the interleaved column of raw
 * row c: bias is indexed like the columns, gm and mag (f32 [C]) in raw order.  No atomics: the bits repeat from launch to launch */
int mrisr_op_dora_mag_grad(int dtype, const void* P, int ldp, const void* Y, int ldy, const void* R, int ldr, const float* bias, const float* mag,
                           float* gm, int M, int C, int geglu_half, void* stream);
/* identity attention (the perturbed rows of mrisr_model_set_pag): vt [B*H][dpad][npad] (T, head-major v^T) -> token rows out [B][N][H*hd]
 * for samples first_sample .. first_sample + n_samples - 1: out[b][t][h*hd + d] = vt[b*H + h][d][t].  A copy: pad columns never reach out, rows
 * of other samples are not written.  Refused before any launch: null or misaligned pointers, npad < N, dpad < hd, a range outside B. */
int mrisr_op_attn_identity(int dtype, const void* vt, void* out, int B, int H, int N, int hd, int npad, int dpad, int first_sample, int n_samples,
                           void* stream);
/* FreeU on one decoder stage's operands alone (the launch mrisr_model_set_freeu adds): NHWC hidden [B][H][W][Ch] and skip [B][H][W][Cs]
 * of `dtype`; hidden_out = hidden with channels [0, Ch / 2) times b, skip_out = fourier_filter(skip, 1, s).  An out pointer may equal its
 * in pointer (in place); buffers must not overlap otherwise.  Refused before any launch: null or not 16-byte aligned pointers, B, H or
 * W < 1 (or H, W > 1024), Ch % 16 != 0, Cs % 8 != 0, b or s negative or not finite. */
int mrisr_op_freeu(int dtype, const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs,
                   float b, float s, void* stream);
/* the same launch with (b, s) of stage `stage` (0: b1, s1; 1: b2, s2) read by the kernel from row `slot` of a host schedule table of n_rows
 * rows (mrisr_sampler_set_schedule's layout and value checks; uploaded here) */
int mrisr_op_freeu_scheduled(int dtype, const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs,
                             int stage, const float* sched_host, int n_rows, int slot, void* stream);
/* the multi-tensor scaled add of the conditioning table alone: for k < n_pairs (1 .. 16), one launch,
 *     x_k[j] = round_T( fma(f_k, r_k[j], x_k[j]) )    f_k = weights[k] * table[4 * slot + col]  (f32, rounded once); table_host NULL: f_k = weights[k]
 * on rows [row_lo, row_hi) of x_k, which has per_row[k] elements of `dtype` per row (and at least row_hi rows); r_k has row_hi - row_lo rows.
 * Rows outside the range are not touched.  table_host: n_rows rows of 4 floats (mrisr_sampler_set_conditioning's layout and checks; uploaded
 * here); col 0 (c) or 1 (a).  Pairs whose two pointers (x_k at row_lo) are 16-byte aligned run in 16-byte pieces with a scalar tail, the
 * others element by element.  Refused before any launch: null pointers, pointers not aligned to the element, an empty pair or row range,
 * a weight that is not finite. */
int mrisr_op_cond_add(int dtype, int n_pairs, void* const* x, const void* const* r, const int64_t* per_row, const float* weights,
                      const float* table_host, int n_rows, int slot, int col, int row_lo, int row_hi, void* stream);
/* the consistency launch of mrisr_sampler_set_consistency alone, on device pointers: x [B,C,h,w] f32 (in place), xK [K B,C,h,w] f32 or NULL
 * (every one of its K parts receives the new x; K = 1 .. 3, NULL only with K = 1), ref [B,C,h,w], lr [B,C,h,w] or NULL, noise
 * [*step + 1 or more][B,C,h,w] or NULL, table_dev [rows][4] = {w, alpha, beta, sigma} and step_dev (one int: the row and slab the kernel
 * reads) on the device.  Operands that are all 16-byte aligned with w % 4 == 0 take the 16-byte path, others the scalar one: same bits.
 * Refused before any launch: null x / ref / table / step, K outside 1 .. 3, a factor outside 2 .. 8 or not dividing h and w, a filter other
 * than 0 / 1, an LDS need above 64 KB, pointers not 4-byte aligned. */
int mrisr_op_consistency(float* x, float* xK, int K, const float* ref, const float* lr, const float* noise, const float* table_dev,
                         const int* step_dev, int B, int C, int h, int w, int factor, int filter, void* stream);
/* dst[z][c][r] = src[z][r][c] for r < r_valid, 0 for r_valid <= r < R (T; pitches ld_src >= C, ld_dst >= R; batch strides in elements) */
int mrisr_op_transpose(int dtype, const void* src, void* dst, int R, int C, int ld_src, int ld_dst, int64_t bs_src, int64_t bs_dst,
                       int batch, int r_valid, void* stream);
/* dS = scale * P o (dP - rowsum(dP o P)) on rows of pitch ld: P (T), dP (f32) -> dS (T); columns nk .. ld-1 of dS are zeroed */
int mrisr_op_softmax_bwd(int dtype, const void* p, const float* dp, void* ds, int ld, int64_t rows, int nk, float scale, void* stream);
/* the tiny dense layers of the time-embedding MLP (rows <= 64, f32 activations).  which = 0: out[N][K] += dY^T act(X), gB[N] += colsum(dY)
 * (xw = X f32 [rows][ldx]; act = SiLU when silu_in; gB optional); which = 1: out[rows][ld_out] = (dY W) * (pre ? silu'(pre) : 1)
 * (xw = W [N][K] of type `dtype`; pre f32 [rows][ldpre] optional) */
int mrisr_op_small_dense_bwd(int dtype, int which, const float* dY, int ldy, const void* xw, int ldx, int rows, int N, int K, int silu_in,
                             const float* pre, int ldpre, float* out, float* gB, int ld_out, void* stream);
/* weight / bias gradient of a conv (ks = 3, pad 1) or linear (ks = 1; xB = 1, xH = M, xW = 1): x NHWC [xB][xH][xW][cin_src] (T), dY rows
 * [M][ldy] (T), columns col0 .. col0 + cout_src; gW f32 [cout][cin][ks][ks] and gB f32 [cout] (optional) are added to; cout <= cout_src,
 * cin <= cin_src (zero-padded layers); geglu_half > 0: the rows of dY are in the GEGLU interleave of a projection with cout = 2 * geglu_half */
int mrisr_op_conv_wgrad(int dtype, const void* x, int xB, int xH, int xW, int cin_src, const void* dY, int ldy, int col0, int cout_src,
                        int ks, int stride, float* gW, float* gB, int cout, int cin, int geglu_half, void* stream);
/* input gradient of a 3x3 conv (pad 1): dy NHWC [B][H][W][cout] (T), w f32 [cout][cin][3][3]; mode 0: stride 1, dx [B][H][W][cin];
 * mode 1: stride 2, dx [B][2H][2W][cin]; accumulate: dx += */
int mrisr_op_conv_dgrad(int dtype, const void* dy, int B, int H, int W, int cout, const float* w_oihw_dev, int cin, int mode, void* dx,
                        int accumulate, void* stream);
/* LoRA on a 3x3 conv (peft lora.Conv2d; stride 1, pad 1).  a_dev: lora_A [r][cin][3][3] f32, b_dev: lora_B [cout][r] f32, both on the device.
 * conv_lora_down: z [B*H*W][r] f32 = conv3x3(x, A) on NHWC x of `dtype`; route 0 = planned, else 100 * (waves per pixel group: 1 or 4) +
 * K slabs (bf16).  conv_lora_dgrad: dx NHWC [B][H][W][cin] of `dtype` (+)= the transposed conv of dz [B*H*W][r] f32 (r in 4 / 8 / 12 / 16).
 * conv3x3_lora: y = conv3x3(x, W) + bias + rowvec[image] + scale * B conv3x3(x, A) + resid as the down-projection followed by the conv with
 * the rank-r term in its epilogue; rowvec_dev ([B][cout] f32) and resid may be null; r = 0 (a_dev, b_dev null): no adapter; splitk / tile force the conv's plan as in mrisr_op_conv3x3. */
int mrisr_op_conv_lora_down(int dtype, const void* x_nhwc, int B, int H, int W, int cin, const float* a_dev, int r, float* z, int route,
                            void* stream);
int mrisr_op_conv_lora_dgrad(int dtype, const float* dz, int B, int H, int W, int r, const float* a_dev, int cin, void* dx_nhwc, int accumulate,
                             void* stream);
int mrisr_op_conv3x3_lora(const mrisr_tensor* x, const float* w_oihw_dev, const float* bias_dev, const float* a_dev, const float* b_dev, int r,
                          float scale, const float* rowvec_dev, const mrisr_tensor* resid, int cout, int splitk, int tile, mrisr_tensor* y,
                          void* stream);


/* the fused guided step of mrisr_sampler_run_guided alone: x [B,C,h,w] f32 (in place), x2 [2B,C,h,w] f32 (receives the new x in
 * both halves), eps2 [2B,C,h,w] f32 (unconditional rows, then conditional), lr / noise [B,C,h,w] f32 or NULL (one noise slab),
 * coef_row_host: the step kind's coefficient row on the host - DDIM {cx, ce}; RESSHIFT {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sigma};
 * DDPM {1/sqrt(abar_t), sqrt(1-abar_t)/sqrt(abar_t), x0 coefficient, x_t coefficient, sigma} */
int mrisr_op_guided_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x2, const mrisr_tensor* eps2, const mrisr_tensor* lr,
                         const mrisr_tensor* noise, const float* coef_row_host, float clip, float guidance_scale,
                         float guidance_rescale, void* stream);

/* the three-way fused step of mrisr_sampler_run_pag (with_cfg) alone: as mrisr_op_guided_step with x3 [3B] (receives the new x in all three
 * thirds) and eps3 [3B] = [eps_p; eps_u; eps_c]; pag_scale == 0 gives mrisr_op_guided_step's result on [eps_u; eps_c] */
int mrisr_op_pag_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x3, const mrisr_tensor* eps3, const mrisr_tensor* lr,
                      const mrisr_tensor* noise, const float* coef_row_host, float clip, float guidance_scale, float pag_scale,
                      float guidance_rescale, void* stream);

/* the same for the multistep kinds: mrisr_op_multistep_step's guided form (hist, xc, row_host, solver_order, slot as there) with x3 / eps3 [3B] */
int mrisr_op_pag_multistep_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x3, const mrisr_tensor* eps3, const mrisr_tensor* lr,
                                mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot, float guidance_scale,
                                float pag_scale, float guidance_rescale, void* stream);

/* the guided step with g, s, phi read from a schedule table (mrisr_sampler_set_schedule) alone: K = 2 with pag_alone == 0 is
 * mrisr_op_guided_step's step on [eps_u; eps_c], K = 2 with pag_alone != 0 the step on [eps_p; eps_c] with g = 1 + s of the row, K = 3
 * mrisr_op_pag_step's, for every step kind.  The kernel sees the step counter `slot` and reads row `slot` of sched_host (n_rows rows of 8
 * floats, uploaded here); the rescale kernel runs iff some row has phi > 0.  row_host: the kind's coefficient row (2 / 4 / 5 floats, or 16
 * for the multistep kinds, which take hist / xc / solver_order as mrisr_op_multistep_step does and NULL otherwise).  noise: NULL or
 * slot + 1 slabs [B,C,h,w] - the step reads slab `slot`.  xK / epsK: [K B,C,h,w]. */
int mrisr_op_scheduled_step(int step_kind, int K, int pag_alone, mrisr_tensor* x, mrisr_tensor* xK, const mrisr_tensor* epsK, const mrisr_tensor* lr,
                            const mrisr_tensor* noise, mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot,
                            float clip, const float* sched_host, int n_rows, void* stream);
/* the reduced step (mrisr_sampler_set_skip) alone: as mrisr_op_scheduled_step without a schedule table, eps [B,C,h,w] the conditional
 * prediction; the new x goes to x and to all K parts of xK [K B,C,h,w], history and corrected state as the guided step writes them. */
int mrisr_op_reduced_step(int step_kind, int K, mrisr_tensor* x, mrisr_tensor* xK, const mrisr_tensor* eps, const mrisr_tensor* lr,
                          const mrisr_tensor* noise, mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot,
                          float clip, void* stream);

/* the fused multistep step (MRISR_STEP_UNIPC / MRISR_STEP_DPMSOLVERPP) alone: x [B,C,h,w] f32 (in place), eps [B,C,h,w], lr or NULL,
 * hist [solver_order][B,C,h,w] f32 (x0 predictions; slot `slot` % solver_order is written, the prediction k steps back is read from
 * slot (slot - k) % solver_order), xc [B,C,h,w] (UniPC: previous corrected state in, this step's out; NULL for DPM-Solver++).
 * row_host, 16 floats: {m: z, eps | corrected state: z, eps, xc, h1, h2, h3 | next state: z, eps, xc, h1, h2, h3 | 0, 0} with
 * z = x - lr.  x2 != NULL: the guided form - eps is [2B] (unconditional rows first), x2 [2B] receives the new x in both halves. */
int mrisr_op_multistep_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x2, const mrisr_tensor* eps, const mrisr_tensor* lr,
                            mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot, float guidance_scale,
                            float guidance_rescale, void* stream);

/* the two kernels of tiled sampling alone, on explicit tables: x [NB,C,H,W] f32 NCHW, xt [NB*ky*kx, C, tile_h, tile_w] f32 NCHW;
 * origins_y / origins_x: host int[ky] / [kx]; weights_y / weights_x: host f32 [ky][tile_h] / [kx][tile_w] (normalised tables).  Refused
 * before any launch: null or misaligned (4-byte) pointers, shape mismatches, origins that do not start at 0, increase, leave no gap
 * and end at extent - tile.  gather copies canvas -> tiles; blend sums tiles -> canvas as mrisr_sampler_set_tiles describes. */
int mrisr_op_tile_gather(const mrisr_tensor* x, mrisr_tensor* xt, const int* origins_y, int ky, const int* origins_x, int kx, void* stream);
int mrisr_op_tile_blend(const mrisr_tensor* xt, mrisr_tensor* x, const int* origins_y, int ky, const int* origins_x, int kx,
                        const float* weights_y, const float* weights_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRISR_H */
