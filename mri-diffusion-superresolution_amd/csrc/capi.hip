// C ABI (include/mrisr.h), the product part: thin extern "C" layer over Model (handles, forward, training step, optimiser).  The graph
// sampler lives in sampler.hip, the T2I-Adapter in adapter.hip, the fine-tuning loop in fit.hip, the VAE in vae.hip, the single-op and
// bench entry points in capi_ops.hip.
#include <algorithm>
#include <cmath>

#include "api.h"
#include "model.h"

using namespace mrisr;

struct mrisr_model : public Model {};

extern "C" {

const char* mrisr_last_error(void) { return last_error_cstr(); }
const char* mrisr_version(void) { return "mrisr 0.1 (gfx950)"; }

static int create_model(const mrisr_unet_cfg* cfg, bool cn, mrisr_model** out) {
    API_BEGIN
    MRISR_REQUIRE(cfg && out, "null argument");
    MRISR_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= 4, "num_levels 1..4");
    MRISR_REQUIRE(cfg->compute_dtype == MRISR_F32 || cfg->compute_dtype == MRISR_BF16, "compute dtype f32 or bf16");
    const int bk = cfg->compute_dtype == MRISR_F32 ? 32 : 64;
    for (int i = 0; i < cfg->num_levels; ++i) {
        MRISR_REQUIRE(cfg->block_out_channels[i] % bk == 0, "block_out_channels must be multiples of the 128-byte K tile");
        MRISR_REQUIRE(cfg->block_out_channels[i] % cfg->num_heads == 0 && (cfg->block_out_channels[i] / cfg->num_heads) % 4 == 0,
                      "head dim must be a multiple of 4");
        MRISR_REQUIRE(cfg->block_out_channels[i] % cfg->norm_num_groups == 0, "channels vs norm groups");
    }
    MRISR_REQUIRE(cfg->cross_attention_dim % bk == 0, "cross_attention_dim must be a multiple of the K tile");
    int dev_count = 0;
    MRISR_CHECK_HIP(hipGetDeviceCount(&dev_count));
    MRISR_REQUIRE(dev_count > 0, "no HIP device: libmrisr has no CPU fallback");
    auto* m = new mrisr_model();
    m->cfg = *cfg;
    m->is_controlnet = cn;
    *out = m;
    return 0;
    API_END
}
int mrisr_unet_create(const mrisr_unet_cfg* cfg, mrisr_model** out) { return create_model(cfg, false, out); }
int mrisr_controlnet_create(const mrisr_unet_cfg* cfg, mrisr_model** out) { return create_model(cfg, true, out); }
void mrisr_model_destroy(mrisr_model* m) { delete m; }

int mrisr_model_set_param(mrisr_model* m, const char* key, const float* data, const int64_t* shape, int ndim,
                          int is_device) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->set_param(key, data, shape, ndim, is_device);
    API_END
}
int mrisr_model_set_lora_scale(mrisr_model* m, float scale) {
    MRISR_REQUIRE(m, "null handle");
    m->lora_scale = scale;
    m->finalized = false;
    return 0;
}
int mrisr_model_set_dora(mrisr_model* m, int use_dora) {
    MRISR_REQUIRE(m, "null handle");
    m->dora = use_dora != 0;
    m->finalized = false;
    return 0;
}
int mrisr_model_set_pag(mrisr_model* m, unsigned block_mask, int first_sample, int n_samples) {
    MRISR_REQUIRE(m, "null handle");
    if (n_samples == 0 || block_mask == 0) {  // off
        MRISR_REQUIRE(n_samples >= 0 && first_sample >= 0, "pag: the sample range must not be negative");
        m->pag = PagState();
        return 0;
    }
    MRISR_REQUIRE(!m->is_controlnet, "pag: perturbed-attention guidance belongs to the UNet, not to a ControlNet handle");
    MRISR_REQUIRE(!m->cfg.fp8_attention, "pag: not supported on a UNet built with fp8_attention");
    MRISR_REQUIRE(!m->keep, "pag: a training forward is being recorded");
    MRISR_REQUIRE(first_sample >= 0 && n_samples > 0, "pag: the sample range must not be negative");
    const int nb = m->num_transformer_blocks();
    MRISR_REQUIRE(nb >= 32 || (block_mask >> nb) == 0, "pag: block_mask selects blocks the UNet does not have (mrisr_model_num_transformer_blocks)");
    m->pag.mask = block_mask; m->pag.first = first_sample; m->pag.count = n_samples;
    return 0;
}
int mrisr_model_set_freeu(mrisr_model* m, int on, float s1, float s2, float b1, float b2) {
    MRISR_REQUIRE(m, "null handle");
    if (!on) {
        m->freeu = FreeUState();
        return 0;
    }
    MRISR_REQUIRE(!m->is_controlnet, "freeu: FreeU belongs to the UNet's decoder, not to a ControlNet handle");
    MRISR_REQUIRE(!m->keep, "freeu: a training forward is being recorded");
    MRISR_REQUIRE(std::isfinite(s1) && s1 >= 0.f, "freeu: s1 must be finite and >= 0");
    MRISR_REQUIRE(std::isfinite(s2) && s2 >= 0.f, "freeu: s2 must be finite and >= 0");
    MRISR_REQUIRE(std::isfinite(b1) && b1 >= 0.f, "freeu: b1 must be finite and >= 0");
    MRISR_REQUIRE(std::isfinite(b2) && b2 >= 0.f, "freeu: b2 must be finite and >= 0");
    m->freeu.on = true;
    m->freeu.s[0] = s1; m->freeu.s[1] = s2; m->freeu.b[0] = b1; m->freeu.b[1] = b2;
    return 0;
}
int mrisr_model_num_transformer_blocks(const mrisr_model* m) { return m ? m->num_transformer_blocks() : 0; }
int mrisr_model_finalize(mrisr_model* m, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    TRY(gemm_prepare());
    return m->finalize((hipStream_t)stream);
    API_END
}
int64_t mrisr_model_num_params(const mrisr_model* m) { return m ? m->num_params() : 0; }
int64_t mrisr_model_workspace_bytes(const mrisr_model* m) {
    return m ? (int64_t)(m->arena.buf.bytes + m->persist.bytes) : 0;
}
int mrisr_model_num_skips(const mrisr_model* m) { return m ? m->num_skips() : 0; }
int mrisr_model_skip_shape(const mrisr_model* m, int k, int B, int h, int w, int64_t shape[4]) {
    MRISR_REQUIRE(m, "null handle");
    return m->skip_shape(k, B, h, w, shape);
}

int mrisr_unet_forward(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep,
                       const mrisr_tensor* ehs, const mrisr_tensor* down_res, int n_down_res,
                       const mrisr_tensor* mid_res, const mrisr_tensor* intrablock, int n_intrablock,
                       mrisr_tensor* out, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->forward_unet(sample, timestep, ehs, down_res, n_down_res, mid_res, intrablock, n_intrablock, out,
                           (hipStream_t)stream);
    API_END
}
int mrisr_unet_cache_shape(const mrisr_model* m, int depth, int B, int h, int w, int64_t shape[4]) {
    MRISR_REQUIRE(m && shape, "null argument");
    MRISR_REQUIRE(!m->is_controlnet, "not a UNet handle");
    return m->cache_shape(depth, B, h, w, shape);
}
int mrisr_unet_forward_cached(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                              const mrisr_tensor* intrablock, int n_intrablock, int depth, int shallow, mrisr_tensor* cache,
                              mrisr_tensor* out, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m && sample && cache, "null argument");
    MRISR_REQUIRE(!m->is_controlnet, "not a UNet handle");
    MRISR_REQUIRE(!m->freeu.on, "FreeU together with a feature cache is not supported (mrisr_model_set_freeu)");
    MRISR_REQUIRE(sample->ndim == 4, "sample must be [B, in_channels, h, w]");
    int64_t cs[4];
    TRY(m->cache_shape(depth, (int)sample->shape[0], (int)sample->shape[2], (int)sample->shape[3], cs));
    // the forward copies cs[0] * ... * cs[3] elements of the compute dtype to / reads them from cache->data without further checks
    MRISR_REQUIRE(cache->data && cache->ndim == 4 && cache->layout == MRISR_NHWC && cache->dtype == m->cfg.compute_dtype,
                  "feature cache: an NHWC tensor in the compute dtype");
    MRISR_REQUIRE(cache->shape[0] == cs[0] && cache->shape[1] == cs[1] && cache->shape[2] == cs[2] && cache->shape[3] == cs[3],
                  "feature cache: shape differs from mrisr_unet_cache_shape");
    UNetCache fc;
    fc.mode = shallow ? CACHE_USE : CACHE_STORE;
    fc.depth = depth;
    fc.p = cache->data;
    return m->forward_unet(sample, timestep, ehs, nullptr, 0, nullptr, intrablock, n_intrablock, out, (hipStream_t)stream, &fc);
    API_END
}
int mrisr_model_set_context(mrisr_model* m, const mrisr_tensor* ehs, int latent_h, int latent_w, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m && ehs, "null argument");
    return m->set_context(ehs, (int)ehs->shape[0], latent_h, latent_w, (hipStream_t)stream);
    API_END
}
int mrisr_controlnet_forward(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep,
                             const mrisr_tensor* ehs, const mrisr_tensor* cond, float conditioning_scale,
                             mrisr_tensor* down_out, int n_down_out, mrisr_tensor* mid_out, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->forward_controlnet(sample, timestep, ehs, cond, conditioning_scale, down_out, n_down_out, mid_out,
                                 (hipStream_t)stream);
    API_END
}
// One forward on the row window [row_lo, row_hi) of the batch the handle's workspace is planned for: `sample` carries the
// window's rows; the context (ControlNet: and the condition image) is the one cached for the full batch; nothing is planned again.
// UNet: down / mid (n_down of them, or 0 / NULL) and the features are inputs at the window's rows, `out` the prediction.
// ControlNet: down / mid are the outputs; no features, no `out`.
int mrisr_model_forward_rows(mrisr_model* m, int row_lo, int row_hi, const mrisr_tensor* sample, const mrisr_tensor* timestep, mrisr_tensor* down,
                             int n_down, mrisr_tensor* mid, const mrisr_tensor* intrablock, int n_intrablock, mrisr_tensor* out, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m && sample && timestep, "null argument");
    const RowWindow rows{row_lo, row_hi};
    if (m->is_controlnet) {
        MRISR_REQUIRE(down && mid && n_intrablock == 0 && !out, "row window: a ControlNet takes its outputs and nothing else");
        return m->forward_controlnet(sample, timestep, nullptr, nullptr, 1.0f, down, n_down, mid, (hipStream_t)stream, &rows);
    }
    MRISR_REQUIRE(out, "row window: a UNet needs its output tensor");
    return m->forward_unet(sample, timestep, nullptr, down, n_down, mid, intrablock, n_intrablock, out, (hipStream_t)stream, nullptr, &rows);
    API_END
}
int mrisr_controlnet_set_cond(mrisr_model* m, const mrisr_tensor* cond, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m && cond, "null argument");
    MRISR_REQUIRE(m->ctx_len > 0, "set the context (or run one forward) before caching the condition image");
    return m->set_cond(cond, m->ctx_len, (hipStream_t)stream);
    API_END
}

int mrisr_resshift_forward(const mrisr_tensor* hr, const mrisr_tensor* lr, const mrisr_tensor* noise,
                           const float* alphas_cumprod_dev, const mrisr_tensor* timestep, mrisr_tensor* out,
                           void* stream) {
    API_BEGIN
    MRISR_REQUIRE(hr && lr && noise && out && timestep && alphas_cumprod_dev, "null argument");
    MRISR_REQUIRE(hr->dtype == MRISR_F32 && lr->dtype == MRISR_F32 && noise->dtype == MRISR_F32 && out->dtype == MRISR_F32,
                  "f32 latents");
    MRISR_REQUIRE(timestep->dtype == MRISR_I64, "int64 timesteps");
    const int B = (int)hr->shape[0];
    long long per = 1;
    for (int i = 1; i < hr->ndim; ++i) per *= hr->shape[i];
    const int scalar = timestep->ndim == 0 || timestep->shape[0] == 1;
    MRISR_REQUIRE(timestep->ndim <= 1 && (scalar || timestep->shape[0] == B), "timesteps: 0-dim, [1] or [B]");
    {
        long long nl = 1, nn = 1, no = 1;
        for (int i = 0; i < lr->ndim; ++i) nl *= lr->shape[i];
        for (int i = 0; i < noise->ndim; ++i) nn *= noise->shape[i];
        for (int i = 0; i < out->ndim; ++i) no *= out->shape[i];
        MRISR_REQUIRE(nl == per * B && nn == per * B && no == per * B, "hr / lr / noise / out must have the same shape");
    }
    return launch_resshift_forward((const float*)hr->data, (const float*)lr->data, (const float*)noise->data,
                                   alphas_cumprod_dev, (const long long*)timestep->data, scalar, (float*)out->data, B,
                                   per, (hipStream_t)stream);
    API_END
}

}  // extern "C"


// ================================================================================================
// LoRA fine-tuning step (train.hip)
// ================================================================================================
extern "C" {

int mrisr_train_prepare(mrisr_model* m, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    TRY(gemm_prepare());
    return m->train_prepare((hipStream_t)stream);
    API_END
}
int64_t mrisr_train_num_trainable(const mrisr_model* m) { return m && m->train_ready ? (int64_t)m->n_trainable : -1; }
int mrisr_train_num_tensors(const mrisr_model* m) { return m && m->train_ready ? (int)m->trainables.size() : -1; }
int mrisr_train_tensor_info(const mrisr_model* m, int i, const char** key, int64_t* offset, int64_t shape[2]) {
    MRISR_REQUIRE(m && m->train_ready, "call mrisr_train_prepare first");
    MRISR_REQUIRE(i >= 0 && i < (int)m->trainables.size() && key && offset && shape, "trainable tensor index");
    const Model::Trainable& t = m->trainables[i];
    *key = t.key.c_str();
    *offset = t.offset;
    shape[0] = t.rows;
    shape[1] = t.cols;
    return 0;
}
int mrisr_train_tensor_shape(const mrisr_model* m, int i, int64_t shape[4], int* ndim) {
    MRISR_REQUIRE(m && m->train_ready, "call mrisr_train_prepare first");
    MRISR_REQUIRE(i >= 0 && i < (int)m->trainables.size() && shape && ndim, "trainable tensor index");
    const Model::Trainable& t = m->trainables[i];
    *ndim = t.ndim;
    if (t.ndim == 2) { shape[0] = t.rows; shape[1] = t.cols; shape[2] = shape[3] = 1; }
    else for (int k = 0; k < 4; ++k) shape[k] = t.shape[k];
    return 0;
}
int mrisr_train_bind(mrisr_model* m, float* theta_dev, float* grad_dev, int init_from_model, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    hipStream_t st = (hipStream_t)stream;
    TRY(m->train_bind(theta_dev, grad_dev, st));
    if (init_from_model) {
        for (auto& t : m->trainables) {
            const RawParam* r = m->find(t.key);
            MRISR_REQUIRE(r && r->numel() == t.numel, "adapter tensor missing from the loaded parameters");
            MRISR_CHECK_HIP(hipMemcpyAsync(theta_dev + t.offset, r->data->p, (size_t)t.numel * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    return m->lora_refresh(st);
    API_END
}
int mrisr_train_refresh(mrisr_model* m, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->lora_refresh((hipStream_t)stream);
    API_END
}
int mrisr_train_step(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                     const mrisr_tensor* intrablock, int n_intrablock, const mrisr_tensor* target, float* loss_dev,
                     mrisr_tensor* pred_out, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->train_step(sample, timestep, ehs, intrablock, n_intrablock, target, loss_dev, pred_out, (hipStream_t)stream);
    API_END
}
int mrisr_train_set_intrablock_grads(mrisr_model* m, const mrisr_tensor* grads, int n) {
    MRISR_REQUIRE(m && n >= 0 && n <= 4 && (n == 0 || grads), "feature-gradient outputs: 0..4 tensors");
    m->d_intra.assign(grads, grads + n);
    return 0;
}
// ---- full-parameter training of a ControlNet handle ----
int mrisr_controlnet_train_prepare(mrisr_model* m, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->full_train_prepare((hipStream_t)stream);
    API_END
}
int64_t mrisr_controlnet_train_num_trainable(const mrisr_model* m) { return m ? m->n_full : 0; }
int mrisr_controlnet_train_num_tensors(const mrisr_model* m) { return m ? (int)m->full_trainables.size() : 0; }
int mrisr_controlnet_train_tensor_info(const mrisr_model* m, int i, const char** key, int64_t* offset, int64_t* numel, int* differentiated) {
    MRISR_REQUIRE(m && i >= 0 && i < (int)m->full_trainables.size() && key && offset && numel, "tensor index");
    const auto& t = m->full_trainables[i];
    *key = t.key.c_str();
    *offset = t.offset;
    *numel = t.numel;
    if (differentiated) *differentiated = std::find(m->full_unsupported.begin(), m->full_unsupported.end(), t.key) == m->full_unsupported.end() ? 1 : 0;
    return 0;
}
int mrisr_controlnet_train_bind(mrisr_model* m, float* theta_dev, float* grad_dev, int init_from_model, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->full_train_bind(theta_dev, grad_dev, init_from_model, (hipStream_t)stream);
    API_END
}
int mrisr_controlnet_train_refresh(mrisr_model* m, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->full_train_refresh((hipStream_t)stream);
    API_END
}
int mrisr_controlnet_train_forward(mrisr_model* m, const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                                   const mrisr_tensor* cond, float conditioning_scale, mrisr_tensor* down_out, int n_down, mrisr_tensor* mid_out,
                                   void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->controlnet_train_forward(sample, timestep, ehs, cond, conditioning_scale, down_out, n_down, mid_out, (hipStream_t)stream);
    API_END
}
int mrisr_controlnet_train_backward(mrisr_model* m, const mrisr_tensor* d_down, int n_down, const mrisr_tensor* d_mid, float conditioning_scale,
                                    void* stream) {
    API_BEGIN
    MRISR_REQUIRE(m, "null handle");
    return m->controlnet_train_backward(d_down, n_down, d_mid, conditioning_scale, (hipStream_t)stream);
    API_END
}
int mrisr_train_set_controlnet_residuals(mrisr_model* m, const mrisr_tensor* down, const mrisr_tensor* d_down, int n_down,
                                         const mrisr_tensor* mid, const mrisr_tensor* d_mid) {
    MRISR_REQUIRE(m && n_down >= 0 && n_down <= 16 && (n_down == 0 || down), "ControlNet residuals of the training step: 0..16 tensors");
    m->tr_down.assign(down, down + n_down);
    if (d_down) m->d_tr_down.assign(d_down, d_down + n_down); else m->d_tr_down.clear();
    m->has_tr_mid = mid != nullptr;
    m->tr_mid = mid ? *mid : mrisr_tensor{};
    m->d_tr_mid = d_mid ? *d_mid : mrisr_tensor{};
    m->train_ws_key.clear();  // the training workspace is planned per residual configuration
    return 0;
}
int mrisr_optim_sumsq(const float* g_dev, int64_t n, float* out_dev, void* stream) {
    MRISR_REQUIRE(g_dev && out_dev && n >= 0, "sumsq arguments");
    return launch_sumsq(g_dev, (long long)n, out_dev, (hipStream_t)stream);
}
int mrisr_optim_ema(float* ema_dev, const float* theta_dev, int64_t n, float decay, void* stream) {
    MRISR_REQUIRE(ema_dev && theta_dev && n >= 0 && decay >= 0.f && decay <= 1.f, "ema arguments");
    return launch_ema(ema_dev, theta_dev, (long long)n, decay, (hipStream_t)stream);
}
int mrisr_optim_adamw(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, const float* sumsq_dev,
                      float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                      int step, void* stream) {
    MRISR_REQUIRE(p_dev && g_dev && m_dev && v_dev && n >= 0 && step >= 1, "adamw arguments");
    MRISR_REQUIRE(max_norm <= 0.f || sumsq_dev, "clipping needs the squared gradient norm");
    return launch_adamw(p_dev, g_dev, m_dev, v_dev, (long long)n, sumsq_dev, grad_scale, max_norm, lr, beta1, beta2, eps,
                        weight_decay, step, (hipStream_t)stream);
}

}  // extern "C"
