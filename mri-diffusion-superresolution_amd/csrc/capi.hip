// C ABI (include/mrisr.h), the product part: thin extern "C" layer over Model (handles, forward, training step, optimiser) plus the
// sampler (per-step hipGraph).  The T2I-Adapter lives in adapter.hip, the fine-tuning loop in fit.hip, the VAE in vae.hip, the
// single-op and bench entry points in capi_ops.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

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

// =================================================================================================
// sampler
// =================================================================================================
__global__ void load_t_kernel(long long* cur_t, const long long* table, const int* step) { *cur_t = table[*step]; }

static int g_temb_table = -1;  // test hook: -1 = MRISR_TEMB_TABLE (default 1), 0 off, 1 on
extern "C" void mrisr_debug_temb_table(int on) { g_temb_table = on; }
static bool temb_table_enabled() {
    static const int env = [] { const char* e = getenv("MRISR_TEMB_TABLE"); return e ? atoi(e) : 1; }();
    return g_temb_table < 0 ? env != 0 : g_temb_table != 0;
}
// ---- multistep solvers (UniPC bh2 / DPM-Solver++ 2M): one row of 16 folded coefficients per step (layout: misc.hip) ----
// rho of the UniPC predictor / corrector: solves the leading k x k block of R rho = b, rows of R = [r_1 .. r_{p-1}, 1]^(j-1),
// b_j = (phi_{j+1}-recurrence value) j! / B(h), B(h) = expm1(-h) (bh2); Gaussian elimination with partial pivoting, k <= 3
static void unipc_rho(const double* rks, int p, double h, int k, double* rho) {
    const double hh = -h, Bh = std::expm1(hh);
    double A[3][4];
    double phik = std::expm1(hh) / hh - 1.0, fact = 1.0;
    for (int j = 1; j <= p; ++j) {
        if (j <= k) {
            for (int c = 0; c < k; ++c) A[j - 1][c] = std::pow(rks[c], j - 1);
            A[j - 1][k] = phik * fact / Bh;
        }
        fact *= j + 1;
        phik = phik / hh - 1.0 / fact;
    }
    for (int c = 0; c < k; ++c) {
        int piv = c;
        for (int r = c + 1; r < k; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        for (int q = 0; q <= k; ++q) std::swap(A[c][q], A[piv][q]);
        for (int r = c + 1; r < k; ++r) {
            const double f = A[r][c] / A[c][c];
            for (int q = c; q <= k; ++q) A[r][q] -= f * A[c][q];
        }
    }
    for (int r = k - 1; r >= 0; --r) {
        double v = A[r][k];
        for (int q = r + 1; q < k; ++q) v -= A[r][q] * rho[q];
        rho[r] = v / A[r][r];
    }
}
struct MultistepOpts {
    int order = 2;
    int final_zero = 1;        // 1: the last step lands on alpha = 1, sigma = 0 (diffusers' "zero"); 0: on alphas_cumprod[0] ("sigma_min")
    int lower_order_final = 1;
    std::vector<int> disable_corrector;  // UniPC: step indices without a corrector
};
// abar: the clamped alphas_cumprod at the n grid timesteps followed by the final point's (ignored when final_zero).  The run starts
// cold at `first`: order 1 and no corrector there.  All arithmetic in double.
static std::vector<float> build_multistep_rows(int kind, const MultistepOpts& o, const std::vector<double>& abar, int n, int first) {
    std::vector<double> al(n + 1), sg(n + 1), lam(n + 1);
    for (int i = 0; i <= n; ++i) {
        al[i] = std::sqrt(abar[i]); sg[i] = std::sqrt(1.0 - abar[i]); lam[i] = std::log(al[i] / sg[i]);
    }
    if (o.final_zero) { al[n] = 1.0; sg[n] = 0.0; lam[n] = INFINITY; }
    auto order_at = [&](int i) {  // order of the predictor step from t_i
        int p = std::min(o.order, i - first + 1);
        if (kind == MRISR_STEP_UNIPC) { if (o.lower_order_final) p = std::min(p, n - i); }
        else if (i == n - 1 && ((o.lower_order_final && n < 15) || o.final_zero)) p = 1;
        return std::max(p, 1);
    };
    std::vector<float> rows((size_t)n * 16, 0.f);
    for (int i = first; i < n; ++i) {
        const double ma = 1.0 / al[i], mb = -sg[i] / al[i];
        // corrected state zc = c[0] z + c[1] eps + c[2] xc + c[3..5] h_1..3      (m = ma z + mb eps folded in)
        double c[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const bool corr = kind == MRISR_STEP_UNIPC && i > first &&
                          std::find(o.disable_corrector.begin(), o.disable_corrector.end(), i) == o.disable_corrector.end();
        if (corr) {
            const int p = order_at(i - 1);
            const double h = lam[i] - lam[i - 1], phi1 = std::expm1(-h), Bh = phi1;
            double rks[3], rho[3] = {0.5, 0.0, 0.0};
            for (int k = 1; k < p; ++k) rks[k - 1] = (lam[i - 1 - k] - lam[i - 1]) / h;
            rks[p - 1] = 1.0;
            if (p > 1) unipc_rho(rks, p, h, p, rho);
            const double cm = -al[i] * Bh * rho[p - 1];
            double ch1 = -al[i] * phi1 + al[i] * Bh * rho[p - 1];
            c[0] = cm * ma; c[1] = cm * mb; c[2] = sg[i] / sg[i - 1];
            for (int k = 1; k < p; ++k) { c[3 + k] = -al[i] * Bh * rho[k - 1] / rks[k - 1]; ch1 += al[i] * Bh * rho[k - 1] / rks[k - 1]; }
            c[3] = ch1;
        }
        // next state from (zc, m, h_1, h_2)
        const int p = order_at(i);
        double pz, pm, ph[3] = {0.0, 0.0, 0.0};
        if (i == n - 1 && o.final_zero) { pz = 0.0; pm = 1.0; }  // h = inf: the state IS the x0 prediction
        else {
            const double h = lam[i + 1] - lam[i], e1 = std::expm1(-h);
            pz = sg[i + 1] / sg[i];
            pm = -al[i + 1] * e1;
            if (kind == MRISR_STEP_UNIPC && p > 1) {
                double rks[3], rho[3] = {0.5, 0.0, 0.0};
                for (int k = 1; k < p; ++k) rks[k - 1] = (lam[i - k] - lam[i]) / h;
                rks[p - 1] = 1.0;
                if (p > 2) unipc_rho(rks, p, h, p - 1, rho);
                for (int k = 1; k < p; ++k) { ph[k - 1] = -al[i + 1] * e1 * rho[k - 1] / rks[k - 1]; pm -= ph[k - 1]; }
            } else if (kind == MRISR_STEP_DPMSOLVERPP && p > 1) {
                const double r0 = (lam[i] - lam[i - 1]) / h;
                ph[0] = 0.5 * al[i + 1] * e1 / r0;
                pm -= ph[0];
            }
        }
        const double nx[6] = {pz * c[0] + pm * ma, pz * c[1] + pm * mb, pz * c[2], pz * c[3] + ph[0], pz * c[4] + ph[1], pz * c[5] + ph[2]};
        float* r = &rows[(size_t)i * 16];
        r[0] = (float)ma; r[1] = (float)mb;
        for (int k = 0; k < 6; ++k) { r[2 + k] = (float)c[k]; r[8 + k] = (float)nx[k]; }
    }
    return rows;
}

struct mrisr_sampler {
    mrisr_model* unet = nullptr;
    mrisr_model* cnet = nullptr;
    int kind = 0, n_steps = 0, first = 0, last = 0;
    float clip = 0.f;
    float guidance_scale = 1.f, guidance_rescale = 0.f;  // classifier-free guidance of mrisr_sampler_run_guided
    unsigned pag_mask = 0;  // perturbed-attention guidance of mrisr_sampler_run_pag: the applied transformer blocks and the scale
    float pag_scale = 0.f;
    int n_captures = 0;     // step graphs captured so far (mrisr_sampler_num_captures)
    std::vector<float> sigma;  // host copy of each step's noise coefficient (which steps read a step_noise slab)
    DevBuf d_ts, d_coef, d_step, d_curt, d_eps;
    // multistep kinds: solver options, the clamped alphas_cumprod on the grid (+ alphas_cumprod[0]), the host rows of the current range,
    // the history ring of `order` x0 predictions and (UniPC) the previous corrected state
    MultistepOpts ms;
    std::vector<double> ms_abar;
    std::vector<float> ms_rows;
    DevBuf d_hist, d_xc;
    bool multistep() const { return kind > MRISR_STEP_DDPM; }
    void rebuild_rows() { if (multistep()) ms_rows = build_multistep_rows(kind, ms, ms_abar, n_steps, first); }
    DevBuf d_x2;  // guided / pag runs: the [K B] f32 latents the forwards read (every part = the state; the fused step keeps them current)
    DevBuf tp_unet, tp_cnet;  // per-run time-embedding tables [scratch | n_steps x tproj_total] (f32)
    std::vector<std::unique_ptr<DevBuf>> res_bufs;   // ControlNet -> UNet residuals (NHWC, compute dtype)
    std::vector<std::unique_ptr<DevBuf>> intra_bufs;  // adapter features converted once
    // feature cache: step i of a run over [first, last) is full (and stores the cache) when (i - first) % interval == 0,
    // shallow (reads it) otherwise; interval 1 = no cache: the body, the key and the graph without it
    int cache_interval = 1, cache_depth = 1;
    DevBuf d_cache;
    // tiled sampling: tile_h == 0 is off.  A run whose grid has more than one tile gathers the state into d_xt
    // [NB*T, C, t_h, t_w], runs the forward there into d_et and blends d_et into d_eps; the grid and the window tables live in d_tiles
    int tile_h = 0, tile_w = 0, tile_oh = 0, tile_ow = 0, tile_window = MRISR_TILE_GAUSSIAN;
    TilePlan tiles;
    DevBuf d_tiles, d_xt, d_et;
    hipGraphExec_t exec = nullptr;
    hipGraphExec_t exec_shallow = nullptr;  // cache_interval > 1: exec is the full + store step, this the shallow one
    std::string graph_key;
    void drop_graphs() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (exec_shallow) (void)hipGraphExecDestroy(exec_shallow);
        exec = exec_shallow = nullptr;
    }
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    ~mrisr_sampler() {
        drop_graphs();
        if (own_stream) (void)hipStreamDestroy(own_stream);
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
    }
};

extern "C" {

int mrisr_sampler_create(mrisr_model* unet, mrisr_model* controlnet, int step_kind, const int64_t* timesteps,
                         int n_steps, const float* alphas_cumprod, int n_train, mrisr_sampler** out) {
    API_BEGIN
    MRISR_REQUIRE(unet && timesteps && alphas_cumprod && out && n_steps > 0, "bad argument");
    MRISR_REQUIRE(!controlnet || controlnet->cfg.compute_dtype == unet->cfg.compute_dtype, "UNet/ControlNet dtype mismatch");
    std::unique_ptr<mrisr_sampler> s(new mrisr_sampler());
    s->unet = unet;
    s->cnet = controlnet;
    s->kind = step_kind;
    s->n_steps = n_steps;
    s->first = 0;
    s->last = n_steps;
    std::vector<long long> ts(timesteps, timesteps + n_steps);
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DPMSOLVERPP, "unknown step kind");
    std::vector<float> coef((size_t)n_steps * (s->multistep() ? 16 : 8), 0.f);
    for (int i = 0; i < n_steps; ++i) {
        const long long t = ts[i];
        MRISR_REQUIRE(t >= 0 && t < n_train, "timestep out of range");
        // zero-terminal-SNR tables (rescale_betas_zero_snr, nb ResDif c11:46) end in abar = 0 exactly and "trailing" spacing
        // samples that entry first: every step divides by sqrt(abar_t) (res_srdiff.py:86), so it is clamped to 2^-24 here
        // (the reference itself would produce inf)
        const double a_t = std::max((double)alphas_cumprod[t], 5.9604644775390625e-8);
        if (s->multistep()) {
            MRISR_REQUIRE(i == 0 || t < ts[i - 1], "multistep solvers need strictly decreasing timesteps");
            s->ms_abar.push_back(a_t);
        } else if (step_kind == MRISR_STEP_DDIM) {
            // t_prev = t - T/n; alpha_prev = alpha[t_prev] or alpha[0] (set_alpha_to_one=False)
            const long long tp = t - n_train / n_steps;
            const double a_p = tp >= 0 ? alphas_cumprod[tp] : alphas_cumprod[0];
            coef[2 * i] = (float)std::sqrt(a_p / a_t);
            coef[2 * i + 1] = (float)(std::sqrt(1.0 - a_p) - std::sqrt(a_p * (1.0 - a_t) / a_t));
        } else if (step_kind == MRISR_STEP_DDPM) {
            // diffusers DDPMScheduler.step, variance_type "fixed_small" (un-vendored; BASELINE config 1)
            const long long tp = t - n_train / n_steps;
            const double a_p = tp >= 0 ? alphas_cumprod[tp] : 1.0;
            const double al = a_t / a_p, be = 1.0 - al;
            coef[8 * i] = (float)(1.0 / std::sqrt(a_t));
            coef[8 * i + 1] = (float)(std::sqrt(1.0 - a_t) / std::sqrt(a_t));
            coef[8 * i + 2] = (float)(std::sqrt(a_p) * be / (1.0 - a_t));
            coef[8 * i + 3] = (float)(std::sqrt(al) * (1.0 - a_p) / (1.0 - a_t));
            coef[8 * i + 4] = t > 0 ? (float)std::sqrt(std::max((1.0 - a_p) / (1.0 - a_t) * be, 1e-20)) : 0.f;
        } else {
            // reference res_srdiff.py:83-96: prev_t = timesteps[i+1] or 0; last step uses alpha[0] and no noise
            const long long tp = i + 1 < n_steps ? ts[i + 1] : 0;
            const double a_p = alphas_cumprod[tp];
            coef[4 * i] = (float)std::sqrt(a_t);
            coef[4 * i + 1] = (float)std::sqrt(1.0 - a_t);
            coef[4 * i + 2] = (float)std::sqrt(a_p);
            coef[4 * i + 3] = tp > 0 ? (float)std::sqrt((1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p)) : 0.f;
        }
    }
    if (s->multistep()) {  // defaults: order 2, diffusers' "zero" final point; mrisr_sampler_set_solver changes them
        s->ms_abar.push_back(std::max((double)alphas_cumprod[0], 5.9604644775390625e-8));
        s->rebuild_rows();
    }
    s->sigma.assign(n_steps, 0.f);
    for (int i = 0; i < n_steps && !s->multistep(); ++i)
        s->sigma[i] = step_kind == MRISR_STEP_DDPM ? coef[8 * i + 4] : (step_kind == MRISR_STEP_RESSHIFT ? coef[4 * i + 3] : 0.f);
    TRY(s->d_ts.reserve(sizeof(long long) * n_steps, false));
    TRY(s->d_coef.reserve(sizeof(float) * coef.size(), false));
    TRY(s->d_step.reserve(16, true));
    TRY(s->d_curt.reserve(16, true));
    MRISR_CHECK_HIP(hipMemcpy(s->d_ts.p, ts.data(), sizeof(long long) * n_steps, hipMemcpyHostToDevice));
    MRISR_CHECK_HIP(hipMemcpy(s->d_coef.p, coef.data(), sizeof(float) * coef.size(), hipMemcpyHostToDevice));
    *out = s.release();
    return 0;
    API_END
}
void mrisr_sampler_destroy(mrisr_sampler* s) { delete s; }
int mrisr_sampler_set_range(mrisr_sampler* s, int first_step, int last_step) {
    API_BEGIN
    MRISR_REQUIRE(s && first_step >= 0 && first_step <= last_step && last_step <= s->n_steps, "step range");
    s->first = first_step;
    s->last = last_step;
    s->rebuild_rows();  // multistep kinds start cold at first_step: order 1, no corrector (allocates: hence the guard)
    return 0;
    API_END
}

int mrisr_sampler_set_solver(mrisr_sampler* s, int solver_order, int final_sigmas_zero, int lower_order_final,
                             const int* disable_corrector, int n_disable) {
    API_BEGIN
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(s->multistep(), "solver options belong to the multistep kinds (UniPC, DPM-Solver++)");
    MRISR_REQUIRE(solver_order >= 1 && solver_order <= (s->kind == MRISR_STEP_UNIPC ? 3 : 2),
                  "solver_order: 1..3 for UniPC, 1..2 for DPM-Solver++");
    MRISR_REQUIRE(lower_order_final == 1, "lower_order_final = false is not implemented");
    MRISR_REQUIRE(n_disable >= 0 && (n_disable == 0 || disable_corrector), "disable_corrector: a list of step indices");
    MRISR_REQUIRE(n_disable == 0 || s->kind == MRISR_STEP_UNIPC, "disable_corrector belongs to UniPC");
    s->ms.order = solver_order;
    s->ms.final_zero = final_sigmas_zero ? 1 : 0;
    s->ms.lower_order_final = 1;
    s->ms.disable_corrector.assign(disable_corrector, disable_corrector + n_disable);
    s->rebuild_rows();
    return 0;
    API_END
}

int mrisr_sampler_set_clip(mrisr_sampler* s, float clip_sample_range) {
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(s->kind == MRISR_STEP_DDPM, "x0 clipping belongs to the DDPM step");
    if (s->clip != clip_sample_range) s->drop_graphs();  // baked into the graph
    s->clip = clip_sample_range;
    return 0;
}

int mrisr_sampler_set_cache(mrisr_sampler* s, int interval, int depth) {
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(interval >= 1, "cache interval must be >= 1 (1: no cache)");
    MRISR_REQUIRE(depth >= 1 && depth <= s->unet->num_skips() - 1, "cache depth must lie in 1 .. num_skips - 1");
    MRISR_REQUIRE(interval == 1 || !s->cnet, "a feature cache together with a ControlNet is not supported");
    MRISR_REQUIRE(interval == 1 || s->tile_h == 0, "a feature cache together with tiles is not supported");
    MRISR_REQUIRE(interval == 1 || !s->unet->freeu.on, "a feature cache together with FreeU is not supported (mrisr_model_set_freeu)");
    if (interval != s->cache_interval || depth != s->cache_depth) s->drop_graphs();  // the next run captures again
    s->cache_interval = interval;
    s->cache_depth = depth;
    return 0;
}

int mrisr_sampler_set_tiles(mrisr_sampler* s, int tile_h, int tile_w, int overlap_h, int overlap_w, int window) {
    MRISR_REQUIRE(s, "null sampler");
    if (tile_h == 0) {  // off: the body, the key and the graph without tiles
        if (s->tile_h) s->drop_graphs();
        s->tile_h = s->tile_w = s->tile_oh = s->tile_ow = 0;
        return 0;
    }
    const int d = 1 << (s->unet->cfg.num_levels - 1);  // the UNet's own divisibility rule for h and w
    MRISR_REQUIRE(tile_h >= d && tile_w >= d && tile_h % d == 0 && tile_w % d == 0, "tile: a multiple of 2^(num_levels-1), at least that");
    MRISR_REQUIRE(overlap_h >= 0 && overlap_w >= 0 && overlap_h < tile_h && overlap_w < tile_w && overlap_h % d == 0 && overlap_w % d == 0,
                  "overlap: a multiple of 2^(num_levels-1) in 0 .. tile - 1");
    MRISR_REQUIRE(window == MRISR_TILE_UNIFORM || window == MRISR_TILE_GAUSSIAN, "window: MRISR_TILE_UNIFORM or MRISR_TILE_GAUSSIAN");
    MRISR_REQUIRE(s->cache_interval == 1, "tiles together with a feature cache are not supported");
    if (tile_h != s->tile_h || tile_w != s->tile_w || overlap_h != s->tile_oh || overlap_w != s->tile_ow || window != s->tile_window)
        s->drop_graphs();
    s->tile_h = tile_h; s->tile_w = tile_w; s->tile_oh = overlap_h; s->tile_ow = overlap_w; s->tile_window = window;
    return 0;
}

int mrisr_sampler_set_guidance(mrisr_sampler* s, float guidance_scale, float guidance_rescale) {
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(std::isfinite(guidance_scale), "guidance_scale must be finite");
    MRISR_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "guidance_rescale must lie in [0, 1]");
    s->guidance_scale = guidance_scale;  // passed to the step kernel by value: part of the graph key
    s->guidance_rescale = guidance_rescale;
    return 0;
}

int mrisr_sampler_set_pag(mrisr_sampler* s, unsigned block_mask, float pag_scale) {
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(std::isfinite(pag_scale) && pag_scale >= 0.f, "pag_scale must be finite and >= 0");
    const int nb = s->unet->num_transformer_blocks();
    MRISR_REQUIRE(nb >= 32 || (block_mask >> nb) == 0, "pag: block_mask selects blocks the UNet does not have (mrisr_model_num_transformer_blocks)");
    MRISR_REQUIRE(pag_scale == 0.f || block_mask != 0, "pag: pag_scale > 0 needs at least one applied block in block_mask");
    s->pag_mask = block_mask;  // both are part of the graph key of the next mrisr_sampler_run_pag
    s->pag_scale = pag_scale;
    return 0;
}
int mrisr_sampler_num_captures(const mrisr_sampler* s) { return s ? s->n_captures : 0; }

// the body of mrisr_sampler_run (K = 1: B rows everywhere), mrisr_sampler_run_guided (K = 2) and mrisr_sampler_run_pag (pag: K = 2 or 3):
// the forwards see NB = K B rows - ehs / cond / intrablock carry K B, the latents are read from the staging buffer; the state, the LR
// anchor and the noise stay [B]
static int sampler_run_impl(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                            const mrisr_tensor* step_noise, const mrisr_tensor* ehs, const mrisr_tensor* cond,
                            const mrisr_tensor* intrablock, int n_intrablock, int use_graph, void* stream, int K, bool pag = false) {
    API_BEGIN
    const bool guided = K > 1;
    MRISR_REQUIRE(s && latents && ehs, "null argument");
    MRISR_REQUIRE(latents->ndim == 4 && latents->dtype == MRISR_F32 && latents->layout == MRISR_NCHW, "latents: f32 NCHW");
    MRISR_REQUIRE(s->kind != MRISR_STEP_RESSHIFT || lr_latents, "Res-SRDiff needs the LR anchor latents");
    MRISR_REQUIRE(!s->multistep() || !step_noise, "the multistep solvers are deterministic: step_noise is refused");
    MRISR_REQUIRE(!s->cnet || cond, "ControlNet needs the condition image");
    const bool cached = s->cache_interval > 1;
    MRISR_REQUIRE(!cached || !s->cnet, "a feature cache together with a ControlNet is not supported");
    MRISR_REQUIRE(!cached || !s->unet->freeu.on, "a feature cache with interval > 1 together with FreeU is not supported (mrisr_model_set_freeu)");
    MRISR_REQUIRE(!s->unet->freeu.on || !s->unet->keep, "FreeU: a training forward is being recorded");
    if (pag) {
        MRISR_REQUIRE(K == 2 || K == 3, "pag run: the forward has 2B rows (pag alone) or 3B rows (with classifier-free guidance)");
        MRISR_REQUIRE(s->pag_mask != 0, "pag run: no applied block (mrisr_sampler_set_pag)");
        MRISR_REQUIRE(!cached, "pag run: a feature cache with interval > 1 is not supported (the shallow pass skips the blocks pag perturbs)");
        MRISR_REQUIRE(!s->unet->cfg.fp8_attention, "pag run: not supported on a UNet built with fp8_attention");
        MRISR_REQUIRE(!s->unet->keep, "pag run: a training forward is being recorded");
    }
    hipStream_t user = (hipStream_t)stream;
    hipStream_t st = user;
    Model& U = *s->unet;
    const int B = (int)latents->shape[0], h = (int)latents->shape[2], w = (int)latents->shape[3];
    const int L = (int)ehs->shape[1];
    const int NB = K * B;  // rows of every forward (of the canvas; a tiled run multiplies them by T)
    const long long per = (long long)latents->shape[1] * h * w;
    const long long n = (long long)B * per;
    const int cdt = U.cfg.compute_dtype;
    const int esz = dtype_size(cdt);
    // every operand the step kernels index is checked against the latents here: the kernels themselves read
    // lr[i], noise[step * n + i] for i < n without bounds
    auto numel = [](const mrisr_tensor* t) { long long k = 1; for (int i = 0; i < t->ndim; ++i) k *= t->shape[i]; return k; };
    MRISR_REQUIRE(latents->shape[1] == U.cfg.in_channels, "latents channels vs the UNet's in_channels");
    // tiles: the grid of this canvas.  T == 1 (or tiles off) is the plain run; otherwise the forwards see FB = NB * T rows of fh x fw
    const int Cl = (int)latents->shape[1];
    bool tiled = false;
    if (s->tile_h) {
        MRISR_REQUIRE(B > 0 && h > 0 && w > 0, "tiled run: empty latents");
        const int d = 1 << (U.cfg.num_levels - 1);
        MRISR_REQUIRE(h % d == 0 && w % d == 0, "tiled run: h and w of the latents must be multiples of 2^(num_levels-1)");
        TRY(s->tiles.build(h, w, s->tile_h, s->tile_w, s->tile_oh, s->tile_ow, s->tile_window));
        TRY(s->tiles.check());
        tiled = s->tiles.T() > 1;
    }
    const int T = tiled ? s->tiles.T() : 1;
    const int fh = tiled ? s->tiles.th : h, fw = tiled ? s->tiles.tw : w;
    if (tiled) MRISR_REQUIRE((long long)NB * T * Cl * fh * fw < (1ll << 31), "tiled run: the tile batch is too large");
    const int FB = NB * T;  // rows of every forward
    if (tiled) {
        MRISR_REQUIRE(!cached, "tiles together with a feature cache are not supported");
        MRISR_REQUIRE(ehs->ndim == 3 && ehs->shape[0] == FB && ehs->shape[2] == U.cfg.cross_attention_dim,
                      "tiled run: encoder_hidden_states must be [NB*T, L, cross_attention_dim]: every forward row's context T times, sample-major");
        if (cond) MRISR_REQUIRE(cond->ndim == 4 && cond->shape[0] == FB && cond->shape[2] == 8 * fh && cond->shape[3] == 8 * fw,
                                "tiled run: controlnet_cond must be [NB*T, C, 8 t_h, 8 t_w]: the image cropped per tile");
        for (int i = 0; i < n_intrablock; ++i) {
            const mrisr_tensor& f = intrablock[i];
            const long long r = f.ndim == 4 && f.shape[2] > 0 ? fh / f.shape[2] : 0;
            MRISR_REQUIRE(f.ndim == 4 && f.shape[0] == FB && r >= 1 && (r & (r - 1)) == 0 && r <= (1ll << (U.cfg.num_levels - 1)) && f.shape[2] * r == fh &&
                              f.shape[3] * r == fw,
                          "tiled run: adapter features must be [NB*T, ...] at tile geometry: every feature cropped per tile");
        }
    } else if (!guided)
        MRISR_REQUIRE(ehs->ndim == 3 && ehs->shape[0] == B && ehs->shape[2] == U.cfg.cross_attention_dim,
                      "encoder_hidden_states must be [B, L, cross_attention_dim] with the latents' batch");
    else
        MRISR_REQUIRE(ehs->ndim == 3 && ehs->shape[0] == NB && ehs->shape[2] == U.cfg.cross_attention_dim,
                      pag ? "pag run: encoder_hidden_states must be [K B, L, cross_attention_dim]: B perturbed rows first, B conditional rows last"
                          : "guided run: encoder_hidden_states must be [2B, L, cross_attention_dim]: B unconditional rows, then B conditional rows");
    if (guided) MRISR_REQUIRE(B > 0 && per % 4 == 0, pag ? "pag run: C*h*w of the latents must be a multiple of 4"
                                                         : "guided run: C*h*w of the latents must be a multiple of 4");
    if (s->multistep()) MRISR_REQUIRE(B > 0 && per % 4 == 0, "multistep solvers: C*h*w of the latents must be a multiple of 4");
    if (lr_latents) MRISR_REQUIRE(lr_latents->dtype == MRISR_F32 && numel(lr_latents) == n, "lr_latents: f32, same shape as latents");
    if (cond && !tiled)
        MRISR_REQUIRE(cond->ndim == 4 && cond->shape[0] == NB && cond->shape[2] == 8 * h && cond->shape[3] == 8 * w,
                      pag ? "pag run: controlnet_cond must be [K B, C, 8h, 8w] (the [B] images K times)"
                      : guided ? "guided run: controlnet_cond must be [2B, C, 8h, 8w] (the [B] images twice)"
                             : "controlnet_cond must be [B, C, 8h, 8w] with the latents' batch");
    {
        int need = 0;  // slabs read: one per step, indexed by the step's position in the schedule, when its sigma != 0
        for (int i = s->first; i < s->last; ++i)
            if (s->sigma[i] != 0.f) need = i + 1;
        if (step_noise) {
            MRISR_REQUIRE(step_noise->dtype == MRISR_F32 && step_noise->ndim >= 1 && numel(step_noise) % n == 0,
                          "step_noise: f32, a stack of latents-shaped slabs");
            MRISR_REQUIRE(numel(step_noise) / n >= need, "step_noise has fewer slabs than the last stochastic step needs");
        }
    }
    for (int i = 0; i < n_intrablock && !tiled; ++i)
        MRISR_REQUIRE(intrablock[i].ndim == 4 && intrablock[i].shape[0] == NB,
                      pag ? "pag run: adapter features must be [K B, ...] (the [B] features K times)"
                      : guided ? "guided run: adapter features must be [2B, ...] (the [B] features twice)"
                             : "adapter features must carry the latents' batch");

    if (use_graph && user == nullptr) {
        // the legacy default stream cannot be captured: run on an internal stream fenced by events
        if (!s->own_stream) {
            MRISR_CHECK_HIP(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
            MRISR_CHECK_HIP(hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming));
            MRISR_CHECK_HIP(hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming));
        }
        st = s->own_stream;
        MRISR_CHECK_HIP(hipEventRecord(s->ev_in, user));
        MRISR_CHECK_HIP(hipStreamWaitEvent(st, s->ev_in, 0));
    }

    // perturbed rows first: samples [0, B) of the forward, [0, B T) of a tiled one.  Set before the workspace is planned (the plan and
    // its key see it), cleared when this call returns, also on an error path: plain forwards on the handle stay unperturbed
    struct PagGuard {
        Model* m = nullptr;
        ~PagGuard() { if (m) m->pag = PagState(); }
    } pguard;
    if (pag) {
        MRISR_REQUIRE(!U.pag.on(), "pag run: the UNet handle already carries a pag state (mrisr_model_set_pag); clear it first");
        pguard.m = &U;
        U.pag.mask = s->pag_mask; U.pag.first = 0; U.pag.count = B * T;
    }
    // ---- one-time (per run) timestep-invariant work: context projections, condition embedding, features ----
    TRY(gemm_prepare());
    TRY(U.set_context(ehs, FB, fh, fw, st));
    std::vector<mrisr_tensor> down_t;
    mrisr_tensor mid_t{};
    int ns = 0;
    if (s->cnet) {
        Model& C = *s->cnet;
        TRY(C.set_context(ehs, FB, fh, fw, st));
        TRY(C.set_cond(cond, L, st));
        ns = C.num_skips();
        s->res_bufs.resize(ns + 1);
        down_t.resize(ns);
        for (int k = 0; k <= ns; ++k) {
            mrisr_tensor t{};
            t.ndim = 4; t.dtype = cdt; t.layout = MRISR_NHWC;
            C.skip_shape(k, FB, fh, fw, t.shape);
            if (!s->res_bufs[k]) s->res_bufs[k].reset(new DevBuf());
            TRY(s->res_bufs[k]->reserve((size_t)t.shape[0] * t.shape[1] * t.shape[2] * t.shape[3] * esz, false));
            t.data = s->res_bufs[k]->p;
            if (k < ns) down_t[k] = t; else mid_t = t;
        }
    }
    std::vector<mrisr_tensor> intra(n_intrablock);
    s->intra_bufs.resize(n_intrablock);
    for (int i = 0; i < n_intrablock; ++i) {
        const mrisr_tensor& f = intrablock[i];
        MRISR_REQUIRE(f.ndim == 4, "adapter feature rank");
        intra[i] = f;
        if (f.layout == MRISR_NHWC && f.dtype == cdt) continue;
        if (!s->intra_bufs[i]) s->intra_bufs[i].reset(new DevBuf());
        TRY(s->intra_bufs[i]->reserve((size_t)f.shape[0] * f.shape[1] * f.shape[2] * f.shape[3] * esz, false));
        if (cdt == MRISR_F32) TRY(launch_nchw_to_nhwc<float>(f.data, f.dtype, s->intra_bufs[i]->p, (int)f.shape[0], (int)f.shape[1], (int)f.shape[2], (int)f.shape[3], st));
        else TRY(launch_nchw_to_nhwc<bf16>(f.data, f.dtype, s->intra_bufs[i]->p, (int)f.shape[0], (int)f.shape[1], (int)f.shape[2], (int)f.shape[3], st));
        intra[i].data = s->intra_bufs[i]->p;
        intra[i].layout = MRISR_NHWC;
        intra[i].dtype = cdt;
    }
    TRY(s->d_eps.reserve((size_t)NB * per * sizeof(float), false));
    TileGrid tg;
    if (tiled) {
        // the table is uploaded before any capture; the graph reads it from d_tiles at every replay.  s->tiles is pageable and rebuilt by the
        // next run: like the copy of ms_rows below, this relies on the runtime staging the copy before hipMemcpyAsync returns
        const size_t tile_elems = (size_t)FB * Cl * fh * fw;
        TRY(s->d_tiles.reserve(s->tiles.bytes(), false));
        TRY(s->d_xt.reserve(tile_elems * sizeof(float), false));
        TRY(s->d_et.reserve(tile_elems * sizeof(float), false));
        MRISR_CHECK_HIP(hipMemcpyAsync(s->d_tiles.p, s->tiles.words.data(), s->tiles.bytes(), hipMemcpyHostToDevice, st));
        tg = s->tiles.grid(s->d_tiles.p);
    }
    UNetCache fc;
    if (cached) {  // reserved here, before any capture; written by the first step of every run before anything reads it
        int64_t cs[4];
        TRY(U.cache_shape(s->cache_depth, NB, h, w, cs));
        TRY(s->d_cache.reserve((size_t)cs[0] * cs[1] * cs[2] * cs[3] * esz, false));
        fc.depth = s->cache_depth;
        fc.p = s->d_cache.p;
    }
    if (guided) {
        // [x; x] ([x; x; x]) once per run; from then on the fused step itself writes every new state to every part
        TRY(s->d_x2.reserve((size_t)K * n * sizeof(float), false));
        for (int k = 0; k < K; ++k)
            MRISR_CHECK_HIP(hipMemcpyAsync(static_cast<float*>(s->d_x2.p) + (size_t)k * n, latents->data, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    // the time embedding of every step of this run, once (it depends on the timestep only): sinusoid -> MLP -> the 22 per-resnet projections for
    // all rows at once instead of three GEMVs over 50 MB of weights in every step.  MRISR_TEMB_TABLE=0 / mrisr_debug_temb_table(0): per step.
    struct TableGuard {  // the models must not keep pointing at this sampler's table after the run (plain forward calls compute their own)
        Model* a = nullptr; Model* b = nullptr;
        ~TableGuard() { if (a) a->tproj_table = nullptr; if (b) b->tproj_table = nullptr; }
    } tguard;
    const bool use_table = temb_table_enabled();
    if (use_table) {
        const int rows = s->last - s->first;
        auto build = [&](Model& M, DevBuf& buf) -> int {
            const size_t scratch = (size_t)64 * M.cfg.block_out_channels[0] * 9;
            TRY(buf.reserve((scratch + (size_t)rows * M.tproj_total) * sizeof(float), false));
            float* sc = static_cast<float*>(buf.p);
            TRY(M.build_tproj_table(static_cast<const long long*>(s->d_ts.p) + s->first, rows, sc, sc + scratch, st));
            M.tproj_table = sc + scratch; M.tproj_step = static_cast<const int*>(s->d_step.p); M.tproj_first = s->first;
            return 0;
        };
        TRY(build(U, s->tp_unet));
        tguard.a = &U;
        if (s->cnet) { TRY(build(*s->cnet, s->tp_cnet)); tguard.b = s->cnet; }
    }
    float* hist = nullptr;
    float* xc = nullptr;
    if (s->multistep()) {
        // this range's rows, and a zeroed history: the rows of a cold start carry zero coefficients for the absent terms, and
        // 0 x (whatever an earlier run or the allocator left) is not 0
        TRY(s->d_hist.reserve((size_t)s->ms.order * n * sizeof(float), false));
        MRISR_CHECK_HIP(hipMemsetAsync(s->d_hist.p, 0, (size_t)s->ms.order * n * sizeof(float), st));
        hist = static_cast<float*>(s->d_hist.p);
        if (s->kind == MRISR_STEP_UNIPC) {
            TRY(s->d_xc.reserve((size_t)n * sizeof(float), false));
            MRISR_CHECK_HIP(hipMemsetAsync(s->d_xc.p, 0, (size_t)n * sizeof(float), st));
            xc = static_cast<float*>(s->d_xc.p);
        }
        // ms_rows is pageable and may be rebuilt (set_solver / set_range) right after this call returns: like the copy of s->first
        // below, this relies on the runtime staging a pageable host-to-device copy before hipMemcpyAsync returns
        MRISR_CHECK_HIP(hipMemcpyAsync(s->d_coef.p, s->ms_rows.data(), sizeof(float) * s->ms_rows.size(), hipMemcpyHostToDevice, st));
    }
    MRISR_CHECK_HIP(hipMemsetAsync(s->d_step.p, 0, 16, st));
    MRISR_CHECK_HIP(hipMemcpyAsync(s->d_step.p, &s->first, sizeof(int), hipMemcpyHostToDevice, st));

    mrisr_tensor tt{};
    tt.data = s->d_curt.p; tt.dtype = MRISR_I64; tt.ndim = 0;
    mrisr_tensor xin = *latents;  // what the forwards read
    if (guided) { xin.shape[0] = NB; xin.data = s->d_x2.p; }
    const float* canvas = static_cast<const float*>(xin.data);  // [NB, C, h, w]: what a tiled step gathers from
    if (tiled) { xin.shape[0] = FB; xin.shape[2] = fh; xin.shape[3] = fw; xin.data = s->d_xt.p; }
    mrisr_tensor eps_t = xin;
    eps_t.data = tiled ? s->d_et.p : s->d_eps.p;
    const int* step = static_cast<const int*>(s->d_step.p);

    auto body = [&](int cache_mode) -> int {
        fc.mode = cache_mode;
        hipLaunchKernelGGL(load_t_kernel, dim3(1), dim3(1), 0, st, static_cast<long long*>(s->d_curt.p),
                           static_cast<const long long*>(s->d_ts.p), step);
        if (tiled) TRY(launch_tile_gather(canvas, static_cast<float*>(s->d_xt.p), tg, NB, Cl, st));
        if (s->cnet)
            TRY(s->cnet->forward_controlnet(&xin, &tt, nullptr, nullptr, 1.0f, down_t.data(), ns, &mid_t, st));
        TRY(U.forward_unet(&xin, &tt, nullptr, s->cnet ? down_t.data() : nullptr, ns, s->cnet ? &mid_t : nullptr,
                           intra.data(), n_intrablock, &eps_t, st, cached ? &fc : nullptr));
        if (tiled) TRY(launch_tile_blend(static_cast<const float*>(s->d_et.p), static_cast<float*>(s->d_eps.p), tg, NB, Cl, st));
        if (K == 3)
            TRY(launch_pag_step(s->kind, (float*)latents->data, (float*)s->d_x2.p, (const float*)s->d_eps.p,
                                lr_latents ? (const float*)lr_latents->data : nullptr, step_noise ? (const float*)step_noise->data : nullptr,
                                (const float*)s->d_coef.p, step, s->clip, s->guidance_scale, s->pag_scale, s->guidance_rescale, B, per, st, hist, xc,
                                s->ms.order));
        else if (pag)  // [eps_p; eps_c]: the guided step with eps_0 := eps_p and g := 1 + s
            TRY(launch_guided_step(s->kind, (float*)latents->data, (float*)s->d_x2.p, (const float*)s->d_eps.p,
                                   lr_latents ? (const float*)lr_latents->data : nullptr, step_noise ? (const float*)step_noise->data : nullptr,
                                   (const float*)s->d_coef.p, step, s->clip, 1.f + s->pag_scale, s->guidance_rescale, B, per, st, hist, xc,
                                   s->ms.order));
        else if (guided)
            TRY(launch_guided_step(s->kind, (float*)latents->data, (float*)s->d_x2.p, (const float*)s->d_eps.p,
                                   lr_latents ? (const float*)lr_latents->data : nullptr, step_noise ? (const float*)step_noise->data : nullptr,
                                   (const float*)s->d_coef.p, step, s->clip, s->guidance_scale, s->guidance_rescale, B, per, st, hist, xc,
                                   s->ms.order));
        else if (s->multistep())
            TRY(launch_multistep_step((float*)latents->data, (const float*)s->d_eps.p, lr_latents ? (const float*)lr_latents->data : nullptr,
                                      (const float*)s->d_coef.p, step, hist, xc, s->ms.order, n, st));
        else if (s->kind == MRISR_STEP_DDIM)
            TRY(launch_ddim_step((float*)latents->data, (const float*)s->d_eps.p, (const float*)s->d_coef.p, step, n, st));
        else if (s->kind == MRISR_STEP_DDPM)
            TRY(launch_ddpm_step((float*)latents->data, (const float*)s->d_eps.p, step_noise ? (const float*)step_noise->data : nullptr,
                                 (const float*)s->d_coef.p, step, s->clip, n, st));
        else
            TRY(launch_resshift_step((float*)latents->data, (const float*)s->d_eps.p, (const float*)lr_latents->data,
                                     step_noise ? (const float*)step_noise->data : nullptr, (const float*)s->d_coef.p, step, n, st));
        return launch_advance_step(static_cast<int*>(s->d_step.p), st);
    };

    auto mode_of = [&](int i) { return !cached ? CACHE_NONE : ((i - s->first) % s->cache_interval == 0 ? CACHE_STORE : CACHE_USE); };
    if (!use_graph) {
        for (int i = s->first; i < s->last; ++i) TRY(body(mode_of(i)));
    } else {
        // everything the captured launches bake in: geometry, caller pointers, the models' workspace generations (persist /
        // arena base addresses change when another geometry, a training step or a second sampler re-plans them), this
        // sampler's own buffers and the feature pointers
        std::string key;
        {
            char kb[256];
            snprintf(kb, sizeof(kb), "%d,%d,%d,%d,%p,%p,%p,%d,g%llu,%llu,e%p", B, h, w, L, latents->data, lr_latents ? lr_latents->data : nullptr,
                     step_noise ? step_noise->data : nullptr, n_intrablock, U.ws_gen, s->cnet ? s->cnet->ws_gen : 0ull, s->d_eps.p);
            key = kb;
            snprintf(kb, sizeof(kb), ",t%p,%p,%d", (const void*)U.tproj_table, s->cnet ? (const void*)s->cnet->tproj_table : nullptr, s->first);
            key += kb;
            for (auto& rb : s->res_bufs) { snprintf(kb, sizeof(kb), ",r%p", rb ? rb->p : nullptr); key += kb; }
            for (auto& f : intra) { snprintf(kb, sizeof(kb), ",f%p", f.data); key += kb; }
            if (guided) {  // the 2B geometry, the staging buffer and the two scalars the guided step takes by value
                snprintf(kb, sizeof(kb), ",G%p,%a,%a", s->d_x2.p, (double)s->guidance_scale, (double)s->guidance_rescale);
                key += kb;
            }
            if (pag) {  // the row count, the applied blocks (also in the UNet's workspace generation) and the scale the step takes by value
                snprintf(kb, sizeof(kb), ",P%d,%x,%a", K, s->pag_mask, (double)s->pag_scale);
                key += kb;
            }
            if (U.freeu.on) {  // the four scalars the decoder's FreeU launches take by value (also in the UNet's workspace generation)
                snprintf(kb, sizeof(kb), ",F%a,%a,%a,%a", (double)U.freeu.s[0], (double)U.freeu.s[1], (double)U.freeu.b[0], (double)U.freeu.b[1]);
                key += kb;
            }
            if (s->multistep()) {  // the ring, the corrected state and the solver order the step takes by value; the other options live in the rows
                snprintf(kb, sizeof(kb), ",M%p,%p,%d,%d,%d", (void*)hist, (void*)xc, s->ms.order, s->ms.final_zero, s->ms.lower_order_final);
                key += kb;
                for (int d : s->ms.disable_corrector) { snprintf(kb, sizeof(kb), ",d%d", d); key += kb; }
            }
            if (cached) {  // the buffer the store node writes and the shallow graph reads, and where the decoder meets it
                snprintf(kb, sizeof(kb), ",C%p,%d", s->d_cache.p, s->cache_depth);
                key += kb;
            }
            if (tiled) {  // the geometry and the window the two kernels take by value or read from the table, the table and the tile batch buffers
                snprintf(kb, sizeof(kb), ",T%d,%d,%d,%d,%d,%p,%p,%p", s->tile_h, s->tile_w, s->tile_oh, s->tile_ow, s->tile_window, s->d_tiles.p,
                         s->d_xt.p, s->d_et.p);
                key += kb;
            }
        }
        if (!s->exec || (cached && !s->exec_shallow) || s->graph_key != key) {
            s->drop_graphs();
            // workspaces are planned (set_context above), so the captured body performs launches only
            auto capture = [&](int cache_mode, hipGraphExec_t* exec) -> int {
                hipGraph_t graph = nullptr;
                MRISR_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                int rc = body(cache_mode);
                hipError_t e = hipStreamEndCapture(st, &graph);
                if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
                MRISR_CHECK_HIP(e);
                MRISR_CHECK_HIP(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
                (void)hipGraphDestroy(graph);
                ++s->n_captures;
                return 0;
            };
            TRY(capture(cached ? CACHE_STORE : CACHE_NONE, &s->exec));
            if (cached) TRY(capture(CACHE_USE, &s->exec_shallow));
            s->graph_key = key;
        }
        for (int i = s->first; i < s->last; ++i) MRISR_CHECK_HIP(hipGraphLaunch(mode_of(i) == CACHE_USE ? s->exec_shallow : s->exec, st));
    }
    if (st != user) {
        MRISR_CHECK_HIP(hipEventRecord(s->ev_out, st));
        MRISR_CHECK_HIP(hipStreamWaitEvent(user, s->ev_out, 0));
    }
    return 0;
    API_END
}

int mrisr_sampler_run(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                      const mrisr_tensor* step_noise, const mrisr_tensor* ehs, const mrisr_tensor* cond,
                      const mrisr_tensor* intrablock, int n_intrablock, int use_graph, void* stream) {
    return sampler_run_impl(s, latents, lr_latents, step_noise, ehs, cond, intrablock, n_intrablock, use_graph, stream, 1);
}
int mrisr_sampler_run_guided(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                             const mrisr_tensor* step_noise, const mrisr_tensor* ehs2, const mrisr_tensor* cond2,
                             const mrisr_tensor* intrablock2, int n_intrablock, int use_graph, void* stream) {
    return sampler_run_impl(s, latents, lr_latents, step_noise, ehs2, cond2, intrablock2, n_intrablock, use_graph, stream, 2);
}
int mrisr_sampler_run_pag(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents, const mrisr_tensor* step_noise,
                          const mrisr_tensor* ehsK, const mrisr_tensor* condK, const mrisr_tensor* intrablockK, int n_intrablock, int with_cfg,
                          int use_graph, void* stream) {
    return sampler_run_impl(s, latents, lr_latents, step_noise, ehsK, condK, intrablockK, n_intrablock, use_graph, stream, with_cfg ? 3 : 2, true);
}

// the three-way step alone, on caller buffers (parity test): as mrisr_op_guided_step with x3 / eps3 [3B] = [perturbed; uncond; cond]
int mrisr_op_pag_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x3, const mrisr_tensor* eps3, const mrisr_tensor* lr,
                      const mrisr_tensor* noise, const float* coef_row_host, float clip, float guidance_scale, float pag_scale,
                      float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && x3 && eps3 && coef_row_host, "pag step: null argument");
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DDPM, "pag step: unknown step kind");
    auto numel = [](const mrisr_tensor* t) { long long k = 1; for (int i = 0; i < t->ndim; ++i) k *= t->shape[i]; return k; };
    MRISR_REQUIRE(x->ndim == 4 && x->dtype == MRISR_F32 && x->shape[0] > 0, "pag step: x must be f32 [B, C, h, w]");
    const int B = (int)x->shape[0];
    const long long n = numel(x), per = n / B;
    MRISR_REQUIRE(x3->dtype == MRISR_F32 && numel(x3) == 3 * n, "pag step: the staging buffer must be f32 [3B, C, h, w]");
    MRISR_REQUIRE(eps3->dtype == MRISR_F32 && numel(eps3) == 3 * n, "pag step: eps3 must be f32 [3B, C, h, w]");
    if (lr) MRISR_REQUIRE(lr->dtype == MRISR_F32 && numel(lr) == n, "pag step: lr must be f32 [B, C, h, w]");
    if (noise) MRISR_REQUIRE(noise->dtype == MRISR_F32 && numel(noise) == n, "pag step: noise must be one f32 [B, C, h, w] slab");
    hipStream_t st = (hipStream_t)stream;
    const int width = step_kind == MRISR_STEP_DDIM ? 2 : (step_kind == MRISR_STEP_RESSHIFT ? 4 : 5);
    float row[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    std::copy(coef_row_host, coef_row_host + width, row);
    DevBuf d_row, d_step;
    TRY(d_row.reserve(sizeof(row), false));
    TRY(d_step.reserve(16, true));  // zeroed: step 0 = the one row, the one noise slab
    MRISR_CHECK_HIP(hipMemcpyAsync(d_row.p, row, sizeof(row), hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemsetAsync(d_step.p, 0, 16, st));
    TRY(launch_pag_step(step_kind, (float*)x->data, (float*)x3->data, (const float*)eps3->data, lr ? (const float*)lr->data : nullptr,
                        noise ? (const float*)noise->data : nullptr, (const float*)d_row.p, (const int*)d_step.p, clip, guidance_scale, pag_scale,
                        guidance_rescale, B, per, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// the guided step alone, on caller buffers (parity test): coef_row_host is this step kind's coefficient row (2 / 4 / 5 floats)
int mrisr_op_guided_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x2, const mrisr_tensor* eps2, const mrisr_tensor* lr,
                         const mrisr_tensor* noise, const float* coef_row_host, float clip, float guidance_scale,
                         float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && x2 && eps2 && coef_row_host, "guided step: null argument");
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DDPM, "guided step: unknown step kind");
    auto numel = [](const mrisr_tensor* t) { long long k = 1; for (int i = 0; i < t->ndim; ++i) k *= t->shape[i]; return k; };
    MRISR_REQUIRE(x->ndim == 4 && x->dtype == MRISR_F32 && x->shape[0] > 0, "guided step: x must be f32 [B, C, h, w]");
    const int B = (int)x->shape[0];
    const long long n = numel(x), per = n / B;
    MRISR_REQUIRE(x2->dtype == MRISR_F32 && numel(x2) == 2 * n, "guided step: the staging buffer must be f32 [2B, C, h, w]");
    MRISR_REQUIRE(eps2->dtype == MRISR_F32 && numel(eps2) == 2 * n, "guided step: eps2 must be f32 [2B, C, h, w]");
    if (lr) MRISR_REQUIRE(lr->dtype == MRISR_F32 && numel(lr) == n, "guided step: lr must be f32 [B, C, h, w]");
    if (noise) MRISR_REQUIRE(noise->dtype == MRISR_F32 && numel(noise) == n, "guided step: noise must be one f32 [B, C, h, w] slab");
    hipStream_t st = (hipStream_t)stream;
    const int width = step_kind == MRISR_STEP_DDIM ? 2 : (step_kind == MRISR_STEP_RESSHIFT ? 4 : 5);
    float row[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    std::copy(coef_row_host, coef_row_host + width, row);
    DevBuf d_row, d_step;
    TRY(d_row.reserve(sizeof(row), false));
    TRY(d_step.reserve(16, true));  // zeroed: step 0 = the one row, the one noise slab
    MRISR_CHECK_HIP(hipMemcpyAsync(d_row.p, row, sizeof(row), hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemsetAsync(d_step.p, 0, 16, st));
    TRY(launch_guided_step(step_kind, (float*)x->data, (float*)x2->data, (const float*)eps2->data, lr ? (const float*)lr->data : nullptr,
                           noise ? (const float*)noise->data : nullptr, (const float*)d_row.p, (const int*)d_step.p, clip,
                           guidance_scale, guidance_rescale, B, per, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// the three-way step of the multistep kinds alone, on caller buffers (parity test): mrisr_op_multistep_step's guided form with x3 / eps3 [3B]
int mrisr_op_pag_multistep_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x3, const mrisr_tensor* eps3, const mrisr_tensor* lr,
                                mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot, float guidance_scale,
                                float pag_scale, float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && x3 && eps3 && hist && row_host, "pag multistep step: null argument");
    MRISR_REQUIRE(step_kind == MRISR_STEP_UNIPC || step_kind == MRISR_STEP_DPMSOLVERPP, "pag multistep step: UniPC or DPM-Solver++");
    MRISR_REQUIRE(solver_order >= 1 && solver_order <= 3 && slot >= 0 && slot < 1024, "pag multistep step: solver order 1..3, slot 0..1023");
    MRISR_REQUIRE((step_kind == MRISR_STEP_UNIPC) == (xc != nullptr), "pag multistep step: the corrected-state buffer belongs to UniPC");
    auto numel = [](const mrisr_tensor* t) { long long k = 1; for (int i = 0; i < t->ndim; ++i) k *= t->shape[i]; return k; };
    MRISR_REQUIRE(x->ndim == 4 && x->dtype == MRISR_F32 && x->shape[0] > 0, "pag multistep step: x must be f32 [B, C, h, w]");
    const int B = (int)x->shape[0];
    const long long n = numel(x), per = n / B;
    MRISR_REQUIRE(per % 4 == 0, "pag multistep step: C*h*w must be a multiple of 4");
    MRISR_REQUIRE(eps3->dtype == MRISR_F32 && numel(eps3) == 3 * n, "pag multistep step: eps3 must be f32 [3B, C, h, w]");
    MRISR_REQUIRE(x3->dtype == MRISR_F32 && numel(x3) == 3 * n, "pag multistep step: the staging buffer must be f32 [3B, C, h, w]");
    if (lr) MRISR_REQUIRE(lr->dtype == MRISR_F32 && numel(lr) == n, "pag multistep step: lr must be f32 [B, C, h, w]");
    MRISR_REQUIRE(hist->dtype == MRISR_F32 && numel(hist) == (long long)solver_order * n, "pag multistep step: hist must be f32 [order, B, C, h, w]");
    if (xc) MRISR_REQUIRE(xc->dtype == MRISR_F32 && numel(xc) == n, "pag multistep step: xc must be f32 [B, C, h, w]");
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> rows((size_t)(slot + 1) * 16, 0.f);
    std::copy(row_host, row_host + 16, rows.begin() + (size_t)slot * 16);
    DevBuf d_rows, d_step;
    TRY(d_rows.reserve(sizeof(float) * rows.size(), false));
    TRY(d_step.reserve(16, true));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_rows.p, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_step.p, &slot, sizeof(int), hipMemcpyHostToDevice, st));
    TRY(launch_pag_step(step_kind, (float*)x->data, (float*)x3->data, (const float*)eps3->data, lr ? (const float*)lr->data : nullptr, nullptr,
                        (const float*)d_rows.p, (const int*)d_step.p, 0.f, guidance_scale, pag_scale, guidance_rescale, B, per, st,
                        (float*)hist->data, xc ? (float*)xc->data : nullptr, solver_order));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// the multistep step alone, on caller buffers (parity test): row_host = one 16-float row; slot = the step counter the kernel sees
int mrisr_op_multistep_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x2, const mrisr_tensor* eps, const mrisr_tensor* lr,
                            mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot, float guidance_scale,
                            float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && eps && hist && row_host, "multistep step: null argument");
    MRISR_REQUIRE(step_kind == MRISR_STEP_UNIPC || step_kind == MRISR_STEP_DPMSOLVERPP, "multistep step: UniPC or DPM-Solver++");
    MRISR_REQUIRE(solver_order >= 1 && solver_order <= 3 && slot >= 0 && slot < 1024, "multistep step: solver order 1..3, slot 0..1023");
    MRISR_REQUIRE((step_kind == MRISR_STEP_UNIPC) == (xc != nullptr), "multistep step: the corrected-state buffer belongs to UniPC");
    auto numel = [](const mrisr_tensor* t) { long long k = 1; for (int i = 0; i < t->ndim; ++i) k *= t->shape[i]; return k; };
    MRISR_REQUIRE(x->ndim == 4 && x->dtype == MRISR_F32 && x->shape[0] > 0, "multistep step: x must be f32 [B, C, h, w]");
    const int B = (int)x->shape[0];
    const long long n = numel(x), per = n / B;
    MRISR_REQUIRE(per % 4 == 0, "multistep step: C*h*w must be a multiple of 4");
    MRISR_REQUIRE(eps->dtype == MRISR_F32 && numel(eps) == (x2 ? 2 : 1) * n, "multistep step: eps must be f32 [B] (plain) or [2B] (guided)");
    if (x2) MRISR_REQUIRE(x2->dtype == MRISR_F32 && numel(x2) == 2 * n, "multistep step: the staging buffer must be f32 [2B, C, h, w]");
    if (lr) MRISR_REQUIRE(lr->dtype == MRISR_F32 && numel(lr) == n, "multistep step: lr must be f32 [B, C, h, w]");
    MRISR_REQUIRE(hist->dtype == MRISR_F32 && numel(hist) == (long long)solver_order * n, "multistep step: hist must be f32 [order, B, C, h, w]");
    if (xc) MRISR_REQUIRE(xc->dtype == MRISR_F32 && numel(xc) == n, "multistep step: xc must be f32 [B, C, h, w]");
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> rows((size_t)(slot + 1) * 16, 0.f);
    std::copy(row_host, row_host + 16, rows.begin() + (size_t)slot * 16);
    DevBuf d_rows, d_step;
    TRY(d_rows.reserve(sizeof(float) * rows.size(), false));
    TRY(d_step.reserve(16, true));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_rows.p, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_step.p, &slot, sizeof(int), hipMemcpyHostToDevice, st));
    if (x2)
        TRY(launch_guided_step(step_kind, (float*)x->data, (float*)x2->data, (const float*)eps->data, lr ? (const float*)lr->data : nullptr,
                               nullptr, (const float*)d_rows.p, (const int*)d_step.p, 0.f, guidance_scale, guidance_rescale, B, per, st,
                               (float*)hist->data, xc ? (float*)xc->data : nullptr, solver_order));
    else
        TRY(launch_multistep_step((float*)x->data, (const float*)eps->data, lr ? (const float*)lr->data : nullptr, (const float*)d_rows.p,
                                  (const int*)d_step.p, (float*)hist->data, xc ? (float*)xc->data : nullptr, solver_order, n, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
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
