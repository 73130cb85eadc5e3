// The fine-tuning loop on the device (mrisr.fit; notebook ResDif c11:14-41 with the reference's batch preparation,
// src/adapters/res_srdiff.py:7-25): a batch builder driven by a counter-based RNG, and the two captured graphs of one optimiser step.
//   graph M (once per micro-batch): batch builder -> train_step (adds into grad) -> loss accumulator, micro counter + 1
//   graph O (once per optimiser step): sumsq (memset node + kernel) -> AdamW from the lr / bias-correction table -> adapter re-pack
//                                      -> EMA from the decay table -> ring writes, step counter + 1 -> grad memset
// Both read the optimiser step s and the micro-batch k from a device counter {s, k}, so one capture of each replays for every step;
// the host only enqueues graph launches (and, with world > 1, the all-reduce of grad between them).
// With a T2I-Adapter (mrisr_fit_create_adapter) graph M also builds the condition (fit_cond_kernel: the item's LR image, 1 -> 3
// channels, PixelUnshuffle(8), straight into the adapter's input activation), runs the adapter forward, hands its features to the
// UNet step and the feature gradients to the adapter backward; graph O clips both buckets by their joint norm and steps both.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "api.h"
#include "model.h"

using namespace mrisr;

struct mrisr_model : public Model {};

namespace {

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11).  Counter = {element group, global sample, step s, k * 8 + stream}, key = seed: every
// (seed, s, k, sample, element, stream) names its own block of four 32-bit words, so a batch is a pure function of (seed, s, k).
// ------------------------------------------------------------------------------------------------
enum : unsigned { RNG_LAT_HR = 0, RNG_LAT_LR = 1, RNG_NOISE = 2, RNG_T = 3, RNG_DROP = 4 };

__device__ inline uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}
__device__ inline uint4 draw(unsigned long long seed, unsigned group, unsigned sample, int s, int k, unsigned stream) {
    return philox4x32_10(make_uint4(group, sample, (unsigned)s, (unsigned)k * 8u + stream),
                         make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
}
// (0, 1]: never 0, so the log of Box-Muller is finite
__device__ inline float u01(unsigned x) { return ((float)(x >> 8) + 1.0f) * (1.0f / 16777216.0f); }
__device__ inline void box_muller(unsigned a, unsigned b, float& z0, float& z1) {
    const float r = sqrtf(-2.0f * logf(u01(a)));
    float sn, cs;
    sincosf(6.283185307179586f * u01(b), &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}
__device__ inline void normal4(unsigned long long seed, unsigned group, unsigned sample, int s, int k, unsigned stream, float z[4]) {
    const uint4 u = draw(seed, group, sample, s, k, stream);
    box_muller(u.x, u.y, z[0], z[1]);
    box_muller(u.z, u.w, z[2], z[3]);
}

struct BatchArgs {
    const float* mom;         // [n_items][4][n]: HR mean, HR std, LR mean, LR std of the VAE posterior (f32)
    const int* index;         // [max_steps * accum][B]: dataset item of every sample of every micro-batch (this rank)
    const int* cap_of_item;   // [n_items]: caption row of each item
    const float* caps;        // [n_captions][row]
    const float* ac;          // alphas_cumprod [T]
    const int* ctr;           // device {s, k} (null: s_fixed / k_fixed)
    int s_fixed, k_fixed, max_steps, accum, B, T, sample_base, empty_row;
    float p_empty, scaling;
    long long n, row;
    unsigned long long seed;
    float* x;                 // noisy latents [B][n]
    float* target;            // eps [B][n]
    long long* t;             // [B]
    float* ehs;               // [B][row]
    float* eps_hr;            // optional: the posterior-sampling noise [B][n]
    float* eps_lr;
    int* cap_row;             // optional: the caption row each sample got [B]
};
__device__ inline void load_sk(const BatchArgs& a, int& s, int& k) {
    s = a.ctr ? a.ctr[0] : a.s_fixed;
    k = a.ctr ? a.ctr[1] : a.k_fixed;
    s = min(max(s, 0), a.max_steps - 1);  // the host never runs past the tables; clamp so a stray counter cannot index out of them
    k = min(max(k, 0), a.accum - 1);
}
__device__ inline int draw_t(const BatchArgs& a, unsigned sample, int s, int k) {
    return (int)__umulhi(draw(a.seed, 0u, sample, s, k, RNG_T).x, (unsigned)a.T);  // floor(u * T), u in [0, 1): uniform on [0, T)
}

// one thread per 4 latent elements of one sample: gather moments, sample z_hr / z_lr, draw eps, res-shift
__global__ __launch_bounds__(256) void fit_latents_kernel(BatchArgs a) {
    const long long groups = (a.n + 3) / 4;
    const long long gid = blockIdx.x * 256ll + threadIdx.x;
    if (gid >= groups * a.B) return;
    const int b = (int)(gid / groups);
    const unsigned g = (unsigned)(gid - (long long)b * groups);
    int s, k;
    load_sk(a, s, k);
    const unsigned sample = (unsigned)(a.sample_base + b);
    const int item = a.index[((long long)s * a.accum + k) * a.B + b];
    const int t = draw_t(a, sample, s, k);
    const float ab = a.ac[t];
    const float ra = sqrtf(ab), rn = sqrtf(1.f - ab);
    float e_hr[4], e_lr[4], eps[4];
    normal4(a.seed, g, sample, s, k, RNG_LAT_HR, e_hr);
    normal4(a.seed, g, sample, s, k, RNG_LAT_LR, e_lr);
    normal4(a.seed, g, sample, s, k, RNG_NOISE, eps);
    const float* m = a.mom + (long long)item * 4 * a.n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = 4ll * g + j;
        if (i >= a.n) break;
        const float z_hr = (m[i] + m[a.n + i] * e_hr[j]) * a.scaling;           // latent_dist.sample() * scaling_factor
        const float z_lr = (m[2 * a.n + i] + m[3 * a.n + i] * e_lr[j]) * a.scaling;
        const long long o = (long long)b * a.n + i;
        a.x[o] = ra * z_hr + (1.f - ra) * z_lr + rn * eps[j];                     // get_res_shifting_latents
        a.target[o] = eps[j];
        if (a.eps_hr) a.eps_hr[o] = e_hr[j];
        if (a.eps_lr) a.eps_lr[o] = e_lr[j];
    }
}

// one thread per caption-embedding element: the sample's caption row, or the empty-prompt row with probability p_empty; t
__global__ __launch_bounds__(256) void fit_context_kernel(BatchArgs a) {
    const long long gid = blockIdx.x * 256ll + threadIdx.x;
    if (gid >= a.row * a.B) return;
    const int b = (int)(gid / a.row);
    const long long e = gid - (long long)b * a.row;
    int s, k;
    load_sk(a, s, k);
    const unsigned sample = (unsigned)(a.sample_base + b);
    const int item = a.index[((long long)s * a.accum + k) * a.B + b];
    int r = a.cap_of_item[item];
    if (a.empty_row >= 0 && u01(draw(a.seed, 0u, sample, s, k, RNG_DROP).x) <= a.p_empty) r = a.empty_row;
    a.ehs[gid] = a.caps[(long long)r * a.row + e];
    if (e == 0) {
        a.t[b] = draw_t(a, sample, s, k);
        if (a.cap_row) a.cap_row[b] = r;
    }
}

// ---- condition builder: LR image table [n_items][res][res] f32 -> the adapter's input ----
struct CondArgs {
    const float* img;        // [n_items][res][res]
    const int* index;
    const int* ctr;
    int s_fixed, k_fixed, max_steps, accum, B, res;
    void* out;
};
__device__ inline void load_sk(const CondArgs& a, int& s, int& k) {
    s = a.ctr ? a.ctr[0] : a.s_fixed;
    k = a.ctr ? a.ctr[1] : a.k_fixed;
    s = min(max(s, 0), a.max_steps - 1);
    k = min(max(k, 0), a.accum - 1);
}
// form 1: u [B][res/8][res/8][192] in the compute dtype, channel c * 64 + dy * 8 + dx = image[8 i + dy][8 j + dx] for c = 0, 1, 2
// (F.pixel_unshuffle(x.expand(3), 8) in NHWC).  One thread per 16 output bytes: V = 16 / sizeof(T) channels of one (c, dy) row,
// read as V contiguous floats of the image row (res % 8 == 0 keeps every read 16-byte aligned).
template <typename T>
__global__ __launch_bounds__(256) void fit_cond_kernel(CondArgs a) {
    constexpr int V = 16 / sizeof(T);
    constexpr int PER_PIX = 192 / V;  // 16-byte chunks per output pixel
    const int h = a.res / 8;
    const long long gid = blockIdx.x * 256ll + threadIdx.x;
    if (gid >= (long long)a.B * h * h * PER_PIX) return;
    const int q = (int)(gid % PER_PIX);
    const long long pix = gid / PER_PIX;
    const int j = (int)(pix % h), i = (int)((pix / h) % h), b = (int)(pix / ((long long)h * h));
    int s, k;
    load_sk(a, s, k);
    const int item = a.index[((long long)s * a.accum + k) * a.B + b];
    const int r = (q * V) % 64, dy = r / 8, dx = r % 8;
    const float* src = a.img + ((long long)item * a.res + (8 * i + dy)) * a.res + 8 * j + dx;
    T* dst = static_cast<T*>(a.out) + pix * 192 + q * V;
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
    } else {
        const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        union { T t[8]; uint4 u; } o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.t[e] = from_f32<T>(v[e]);
        *reinterpret_cast<uint4*>(dst) = o.u;
    }
}
// form 0: x [B][3][res][res] f32 (the input of Adapter_XL.forward): one thread per 4 pixels, the same float4 to each channel
__global__ __launch_bounds__(256) void fit_cond_image_kernel(CondArgs a) {
    const long long plane = (long long)a.res * a.res, groups = plane / 4;
    const long long gid = blockIdx.x * 256ll + threadIdx.x;
    if (gid >= groups * a.B) return;
    const int b = (int)(gid / groups);
    const long long g = gid - (long long)b * groups;
    int s, k;
    load_sk(a, s, k);
    const int item = a.index[((long long)s * a.accum + k) * a.B + b];
    const float4 v = reinterpret_cast<const float4*>(a.img + (long long)item * plane)[g];
    float4* dst = reinterpret_cast<float4*>(static_cast<float*>(a.out) + (long long)b * 3 * plane);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * groups + g] = v;
}

int launch_cond(const CondArgs& a, int form, int dtype, hipStream_t st) {
    const long long h = a.res / 8;
    if (form == 0) {
        const long long n = (long long)a.res * a.res / 4 * a.B;
        hipLaunchKernelGGL(fit_cond_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    } else if (dtype == MRISR_F32) {
        const long long n = (long long)a.B * h * h * (192 / 4);
        hipLaunchKernelGGL(fit_cond_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    } else {
        const long long n = (long long)a.B * h * h * (192 / 8);
        hipLaunchKernelGGL(fit_cond_kernel<bf16>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    }
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_batch(const BatchArgs& a, hipStream_t st) {
    const long long n1 = (a.n + 3) / 4 * a.B, n2 = a.row * a.B;
    hipLaunchKernelGGL(fit_latents_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(fit_context_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, a);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// end of a micro-batch: accumulate its loss, k + 1 (plain stores from one thread)
__global__ void fit_micro_end_kernel(int* ctr, const float* loss, float* loss_acc) {
    *loss_acc += *loss;
    ctr[1] += 1;
}
// end of an optimiser step: ring entries of step s, reset the accumulator, s + 1, k = 0
__global__ void fit_step_end_kernel(int* ctr, float* loss_acc, const float* sumsq, const float* sched, float inv_accum, float grad_scale,
                                    int max_steps, float* loss_ring, float* gnorm_ring, float* lr_ring) {
    const int s = ctr[0];
    if (s >= 0 && s < max_steps) {
        loss_ring[s] = *loss_acc * inv_accum;
        gnorm_ring[s] = sqrtf(*sumsq) * grad_scale;
        lr_ring[s] = sched[3 * s];
    }
    *loss_acc = 0.f;
    ctr[0] = s + 1;
    ctr[1] = 0;
}

}  // namespace

struct mrisr_fit {
    mrisr_model* m = nullptr;
    mrisr_fit_config cfg{};
    long long n = 0, row = 0, n_theta = 0;
    const float* mom = nullptr;
    const float* caps = nullptr;
    float *exp_avg = nullptr, *exp_avg_sq = nullptr, *ema = nullptr;
    float *loss_ring = nullptr, *gnorm_ring = nullptr, *lr_ring = nullptr;
    DevBuf d_index, d_capid, d_ac, d_sched, d_decay, d_ctr, d_x, d_tgt, d_t, d_ehs, d_scalars;
    int host_ctr[4] = {0, 0, 0, 0};  // host mirror of {s, k}; also the source of set_step's copy
    // T2I-Adapter (mrisr_fit_create_adapter; null: the LoRA-only loop)
    mrisr_adapter* ad = nullptr;
    AdapterFitInfo ai{};
    int res = 0;
    const float* cond = nullptr;
    float *ad_exp_avg = nullptr, *ad_exp_avg_sq = nullptr, *ad_ema = nullptr;
    DevBuf d_u, d_feat[4], d_dfeat[4];
    mrisr_tensor u_t{}, feats[4]{}, dfeats[4]{};
    hipGraphExec_t exec_m = nullptr, exec_o = nullptr;
    std::string key_m, key_o;
    int captures = 0;
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    ~mrisr_fit() {
        if (exec_m) (void)hipGraphExecDestroy(exec_m);
        if (exec_o) (void)hipGraphExecDestroy(exec_o);
        if (own_stream) (void)hipStreamDestroy(own_stream);
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_out) (void)hipEventDestroy(ev_out);
    }
    // the legacy default stream cannot be captured: graphs then run on an internal stream fenced by events (as the sampler does)
    int enter(hipStream_t user, hipStream_t* st) {
        *st = user;
        if (user) return 0;
        if (!own_stream) {
            MRISR_CHECK_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
            MRISR_CHECK_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
            MRISR_CHECK_HIP(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
        }
        MRISR_CHECK_HIP(hipEventRecord(ev_in, user));
        MRISR_CHECK_HIP(hipStreamWaitEvent(own_stream, ev_in, 0));
        *st = own_stream;
        return 0;
    }
    int leave(hipStream_t user, hipStream_t st) {
        if (st == user) return 0;
        MRISR_CHECK_HIP(hipEventRecord(ev_out, st));
        MRISR_CHECK_HIP(hipStreamWaitEvent(user, ev_out, 0));
        return 0;
    }
    float* loss() { return static_cast<float*>(d_scalars.p); }
    float* loss_acc() { return static_cast<float*>(d_scalars.p) + 1; }
    float* sumsq() { return static_cast<float*>(d_scalars.p) + 2; }
    int* ctr() { return static_cast<int*>(d_ctr.p); }
    BatchArgs args() const {
        BatchArgs a{};
        a.mom = mom; a.index = static_cast<const int*>(d_index.p); a.cap_of_item = static_cast<const int*>(d_capid.p); a.caps = caps;
        a.ac = static_cast<const float*>(d_ac.p); a.ctr = static_cast<const int*>(d_ctr.p);
        a.max_steps = cfg.max_steps; a.accum = cfg.accum; a.B = cfg.batch; a.T = cfg.num_train_timesteps; a.sample_base = cfg.sample_base;
        a.empty_row = cfg.empty_row; a.p_empty = cfg.proportion_empty; a.scaling = cfg.scaling_factor; a.n = n; a.row = row; a.seed = cfg.seed;
        a.x = static_cast<float*>(d_x.p); a.target = static_cast<float*>(d_tgt.p); a.t = static_cast<long long*>(d_t.p);
        a.ehs = static_cast<float*>(d_ehs.p);
        return a;
    }
    void describe(mrisr_tensor& x, mrisr_tensor& t, mrisr_tensor& e, mrisr_tensor& g) {
        x = mrisr_tensor{}; x.data = d_x.p; x.ndim = 4; x.dtype = MRISR_F32; x.layout = MRISR_NCHW;
        x.shape[0] = cfg.batch; x.shape[1] = cfg.latent_channels; x.shape[2] = cfg.latent_h; x.shape[3] = cfg.latent_w;
        g = x; g.data = d_tgt.p;
        t = mrisr_tensor{}; t.data = d_t.p; t.ndim = 1; t.dtype = MRISR_I64; t.shape[0] = cfg.batch;
        e = mrisr_tensor{}; e.data = d_ehs.p; e.ndim = 3; e.dtype = MRISR_F32; e.layout = MRISR_NCHW;
        e.shape[0] = cfg.batch; e.shape[1] = cfg.ctx_len; e.shape[2] = cfg.ctx_dim;
    }
    CondArgs cond_args() const {
        CondArgs a{};
        a.img = cond; a.index = static_cast<const int*>(d_index.p); a.ctr = static_cast<const int*>(d_ctr.p);
        a.max_steps = cfg.max_steps; a.accum = cfg.accum; a.B = cfg.batch; a.res = res; a.out = u_t.data;
        return a;
    }
    // every address a capture bakes in besides this handle's own buffers (fixed for its lifetime): the model's workspace generation
    // (persist / arena base addresses change when a validation forward or another geometry re-plans them), the bound vectors, the
    // adapter scale the re-pack kernels take by value
    std::string model_key() const {
        char kb[256];
        snprintf(kb, sizeof(kb), "g%llu,a%p,p%p,th%p,gr%p,s%a", m->ws_gen, m->arena.buf.p, m->persist.p, (void*)m->theta, (void*)m->grad,
                 (double)m->lora_scale);
        return kb;
    }
};

static int capture(hipStream_t st, hipGraphExec_t* exec, const std::function<int()>& body) {
    if (*exec) { (void)hipGraphExecDestroy(*exec); *exec = nullptr; }
    hipGraph_t graph = nullptr;
    MRISR_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = body();
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    MRISR_CHECK_HIP(e);
    MRISR_CHECK_HIP(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    return 0;
}

extern "C" {

static int fit_create(mrisr_model* unet, const mrisr_fit_config* cfg, const float* moments_dev, const float* captions_dev,
                      const int32_t* caption_of_item, const int32_t* index_table, const float* alphas_cumprod, const float* lr_table,
                      const float* ema_decay_table, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, float* loss_ring_dev,
                      float* grad_norm_ring_dev, float* lr_ring_dev, const mrisr_fit_adapter_args* ad, mrisr_fit** out) {
    MRISR_REQUIRE(unet && cfg && moments_dev && captions_dev && caption_of_item && index_table && alphas_cumprod && lr_table && out,
                  "null argument");
    MRISR_REQUIRE(loss_ring_dev && grad_norm_ring_dev && lr_ring_dev, "optimiser state / rings");
    Model& U = *unet;
    if (!ad) MRISR_REQUIRE(U.train_ready && U.theta && U.grad && U.n_trainable > 0, "bind the adapters first (mrisr_train_bind; lora_fused = 1)");
    else MRISR_REQUIRE(U.train_ready && (U.n_trainable == 0 || (U.theta && U.grad)), "prepare the UNet for training first (mrisr_train_bind)");
    const bool lora = U.n_trainable > 0;
    MRISR_REQUIRE(!lora || (exp_avg_dev && exp_avg_sq_dev), "optimiser state / rings");
    const mrisr_fit_config& c = *cfg;
    MRISR_REQUIRE(c.batch > 0 && c.accum > 0 && c.max_steps > 0 && c.world > 0 && c.sample_base >= 0, "batch / accum / steps / world");
    MRISR_REQUIRE(c.n_items > 0 && c.n_captions > 0 && c.ctx_len > 0 && c.ctx_dim == U.cfg.cross_attention_dim, "items / captions");
    MRISR_REQUIRE(c.latent_channels == U.cfg.in_channels && c.latent_h > 0 && c.latent_w > 0, "latent geometry");
    MRISR_REQUIRE(c.num_train_timesteps > 0 && c.empty_row >= -1 && c.empty_row < c.n_captions, "timesteps / empty row");
    MRISR_REQUIRE(c.proportion_empty >= 0.f && c.proportion_empty <= 1.f && (c.proportion_empty == 0.f || c.empty_row >= 0),
                  "proportion_empty_prompts needs the empty-prompt row");
    MRISR_REQUIRE(!c.use_ema || ((ema_dev || !lora) && ema_decay_table), "EMA needs its vector and decay table");
    AdapterFitInfo ai{};
    if (ad) {
        MRISR_REQUIRE(ad->adapter && ad->cond_dev && ad->exp_avg_dev && ad->exp_avg_sq_dev && (!c.use_ema || ad->ema_dev),
                      "adapter: handle, condition table, optimiser state");
        TRY(adapter_fit_info(ad->adapter, &ai));
        MRISR_REQUIRE(ai.n_trainable > 0 && ai.theta && ai.grad, "bind the adapter's trainable vector first (mrisr_adapter_train_bind)");
        MRISR_REQUIRE(ai.compute_dtype == U.cfg.compute_dtype, "the adapter's compute dtype differs from the UNet's");
        MRISR_REQUIRE(ai.cin == 192, "the condition builder feeds cin = 192 (3 channels, PixelUnshuffle(8))");
        MRISR_REQUIRE(ad->res > 0 && ad->res % 8 == 0, "condition resolution must be a multiple of 8");
        MRISR_REQUIRE(ad->res / 8 == c.latent_h && ad->res / 8 == c.latent_w, "condition resolution / 8 must equal the latent size");
        // one feature per UNet level, of that level's channels and size (stride-2 convs on both sides: (n - 1) / 2 + 1)
        MRISR_REQUIRE(ai.n_levels == U.cfg.num_levels && ai.n_levels <= 4, "adapter levels must equal the UNet's down levels");
        for (int i = 0; i < ai.n_levels; ++i)
            MRISR_REQUIRE(ai.channels[i] == U.cfg.block_out_channels[i], "adapter feature channels do not match the UNet's intrablock positions");
    }
    // every index the kernels follow unchecked is checked here once
    const long long n_idx = (long long)c.max_steps * c.accum * c.batch;
    for (long long i = 0; i < n_idx; ++i) MRISR_REQUIRE(index_table[i] >= 0 && index_table[i] < c.n_items, "index table entry out of range");
    for (int i = 0; i < c.n_items; ++i)
        MRISR_REQUIRE(caption_of_item[i] >= 0 && caption_of_item[i] < c.n_captions, "caption row out of range");
    std::unique_ptr<mrisr_fit> f(new mrisr_fit());
    f->m = unet;
    f->cfg = c;
    f->n = (long long)c.latent_channels * c.latent_h * c.latent_w;
    f->row = (long long)c.ctx_len * c.ctx_dim;
    f->n_theta = U.n_trainable;
    f->mom = moments_dev;
    f->caps = captions_dev;
    f->exp_avg = exp_avg_dev;
    f->exp_avg_sq = exp_avg_sq_dev;
    f->ema = c.use_ema ? ema_dev : nullptr;
    f->loss_ring = loss_ring_dev;
    f->gnorm_ring = grad_norm_ring_dev;
    f->lr_ring = lr_ring_dev;
    // {lr, 1 - b1^step, 1 - b2^step} of every optimiser step: the same float expressions launch_adamw evaluates per call
    std::vector<float> sched((size_t)c.max_steps * 3);
    for (int s = 0; s < c.max_steps; ++s) {
        sched[3 * s] = lr_table[s];
        sched[3 * s + 1] = 1.0f - powf(c.beta1, (float)(s + 1));
        sched[3 * s + 2] = 1.0f - powf(c.beta2, (float)(s + 1));
    }
    TRY(f->d_index.reserve(sizeof(int) * n_idx, false));
    TRY(f->d_capid.reserve(sizeof(int) * c.n_items, false));
    TRY(f->d_ac.reserve(sizeof(float) * c.num_train_timesteps, false));
    TRY(f->d_sched.reserve(sizeof(float) * sched.size(), false));
    TRY(f->d_ctr.reserve(16, true));
    TRY(f->d_scalars.reserve(16, true));
    TRY(f->d_x.reserve(sizeof(float) * c.batch * f->n, false));
    TRY(f->d_tgt.reserve(sizeof(float) * c.batch * f->n, false));
    TRY(f->d_t.reserve(sizeof(long long) * c.batch, false));
    TRY(f->d_ehs.reserve(sizeof(float) * c.batch * f->row, false));
    MRISR_CHECK_HIP(hipMemcpy(f->d_index.p, index_table, sizeof(int) * n_idx, hipMemcpyHostToDevice));
    MRISR_CHECK_HIP(hipMemcpy(f->d_capid.p, caption_of_item, sizeof(int) * c.n_items, hipMemcpyHostToDevice));
    MRISR_CHECK_HIP(hipMemcpy(f->d_ac.p, alphas_cumprod, sizeof(float) * c.num_train_timesteps, hipMemcpyHostToDevice));
    MRISR_CHECK_HIP(hipMemcpy(f->d_sched.p, sched.data(), sizeof(float) * sched.size(), hipMemcpyHostToDevice));
    if (c.use_ema) {
        TRY(f->d_decay.reserve(sizeof(float) * c.max_steps, false));
        MRISR_CHECK_HIP(hipMemcpy(f->d_decay.p, ema_decay_table, sizeof(float) * c.max_steps, hipMemcpyHostToDevice));
    }
    if (ad) {
        f->ad = ad->adapter;
        f->ai = ai;
        f->res = ad->res;
        f->cond = ad->cond_dev;
        f->ad_exp_avg = ad->exp_avg_dev;
        f->ad_exp_avg_sq = ad->exp_avg_sq_dev;
        f->ad_ema = c.use_ema ? ad->ema_dev : nullptr;
        const int cdt = U.cfg.compute_dtype;
        const size_t es = dtype_size(cdt);
        const int h = ad->res / 8;
        mrisr_tensor& u = f->u_t;
        u.ndim = 4; u.dtype = cdt; u.layout = MRISR_NHWC;
        u.shape[0] = c.batch; u.shape[1] = 192; u.shape[2] = h; u.shape[3] = h;  // logical [B, C, H, W], stored NHWC
        TRY(f->d_u.reserve((size_t)c.batch * h * h * 192 * es, false));
        u.data = f->d_u.p;
        int hh = h;
        for (int i = 0; i < ai.n_levels; ++i) {
            if (i) hh = (hh - 1) / 2 + 1;
            mrisr_tensor t{};
            t.ndim = 4; t.dtype = cdt; t.layout = MRISR_NHWC;
            t.shape[0] = c.batch; t.shape[1] = ai.channels[i]; t.shape[2] = hh; t.shape[3] = hh;  // logical [B, C, H, W], stored NHWC
            const size_t bytes = (size_t)c.batch * ai.channels[i] * hh * hh * es;
            TRY(f->d_feat[i].reserve(bytes, false));
            TRY(f->d_dfeat[i].reserve(bytes, false));
            f->feats[i] = t;
            f->feats[i].data = f->d_feat[i].p;
            f->dfeats[i] = t;
            f->dfeats[i].data = f->d_dfeat[i].p;
        }
    }
    *out = f.release();
    return 0;
}

int mrisr_fit_create(mrisr_model* unet, const mrisr_fit_config* cfg, const float* moments_dev, const float* captions_dev,
                     const int32_t* caption_of_item, const int32_t* index_table, const float* alphas_cumprod, const float* lr_table,
                     const float* ema_decay_table, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, float* loss_ring_dev,
                     float* grad_norm_ring_dev, float* lr_ring_dev, mrisr_fit** out) {
    API_BEGIN
    return fit_create(unet, cfg, moments_dev, captions_dev, caption_of_item, index_table, alphas_cumprod, lr_table, ema_decay_table,
                      exp_avg_dev, exp_avg_sq_dev, ema_dev, loss_ring_dev, grad_norm_ring_dev, lr_ring_dev, nullptr, out);
    API_END
}

int mrisr_fit_create_adapter(mrisr_model* unet, const mrisr_fit_config* cfg, const float* moments_dev, const float* captions_dev,
                             const int32_t* caption_of_item, const int32_t* index_table, const float* alphas_cumprod,
                             const float* lr_table, const float* ema_decay_table, float* exp_avg_dev, float* exp_avg_sq_dev,
                             float* ema_dev, float* loss_ring_dev, float* grad_norm_ring_dev, float* lr_ring_dev,
                             const mrisr_fit_adapter_args* adapter, mrisr_fit** out) {
    API_BEGIN
    MRISR_REQUIRE(adapter, "null adapter arguments");
    return fit_create(unet, cfg, moments_dev, captions_dev, caption_of_item, index_table, alphas_cumprod, lr_table, ema_decay_table,
                      exp_avg_dev, exp_avg_sq_dev, ema_dev, loss_ring_dev, grad_norm_ring_dev, lr_ring_dev, adapter, out);
    API_END
}

void mrisr_fit_destroy(mrisr_fit* f) { delete f; }

int mrisr_fit_set_step(mrisr_fit* f, int step, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(f && step >= 0 && step <= f->cfg.max_steps, "step out of range");
    hipStream_t st = (hipStream_t)stream;
    f->host_ctr[0] = step;
    f->host_ctr[1] = 0;
    MRISR_CHECK_HIP(hipMemcpyAsync(f->d_ctr.p, f->host_ctr, 2 * sizeof(int), hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemsetAsync(f->loss_acc(), 0, sizeof(float), st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));  // host_ctr is the copy's source
    return 0;
    API_END
}

int mrisr_fit_get_step(const mrisr_fit* f) { return f ? f->host_ctr[0] : -1; }
int mrisr_fit_num_captures(const mrisr_fit* f) { return f ? f->captures : -1; }

int mrisr_fit_make_batch(mrisr_fit* f, int step, int micro, float* sample_dev, int64_t* timesteps_dev, float* ehs_dev, float* target_dev,
                         float* eps_hr_dev, float* eps_lr_dev, int32_t* caption_row_dev, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(f && sample_dev && timesteps_dev && ehs_dev && target_dev, "null argument");
    MRISR_REQUIRE(step >= 0 && step < f->cfg.max_steps && micro >= 0 && micro < f->cfg.accum, "(step, micro) outside the run");
    BatchArgs a = f->args();
    a.ctr = nullptr;
    a.s_fixed = step;
    a.k_fixed = micro;
    a.x = sample_dev; a.t = reinterpret_cast<long long*>(timesteps_dev); a.ehs = ehs_dev; a.target = target_dev;
    a.eps_hr = eps_hr_dev; a.eps_lr = eps_lr_dev; a.cap_row = caption_row_dev;
    return launch_batch(a, (hipStream_t)stream);
    API_END
}

int mrisr_fit_make_condition(mrisr_fit* f, int step, int micro, void* out_dev, int form, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(f && out_dev, "null argument");
    MRISR_REQUIRE(f->ad, "the loop trains no T2I-Adapter (mrisr_fit_create_adapter)");
    MRISR_REQUIRE(form == 0 || form == 1, "form 0 (NCHW f32 image) or 1 (unshuffled NHWC activation)");
    MRISR_REQUIRE(step >= 0 && step < f->cfg.max_steps && micro >= 0 && micro < f->cfg.accum, "(step, micro) outside the run");
    CondArgs a = f->cond_args();
    a.ctr = nullptr;
    a.s_fixed = step;
    a.k_fixed = micro;
    a.out = out_dev;
    return launch_cond(a, form, f->ai.compute_dtype, (hipStream_t)stream);
    API_END
}

int mrisr_fit_micro(mrisr_fit* f, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(f, "null handle");
    MRISR_REQUIRE(f->host_ctr[0] < f->cfg.max_steps && f->host_ctr[1] < f->cfg.accum, "micro-batch outside the run (max_train_steps / accum)");
    hipStream_t user = (hipStream_t)stream, st;
    TRY(f->enter(user, &st));
    Model& U = *f->m;
    // a plain training step of this model may have left T2I-Adapter / ControlNet hooks set: the loop trains the LoRA UNet alone,
    // or with this handle's adapter, whose feature gradients go to the handle's own buffers
    const int n_feats = f->ad ? f->ai.n_levels : 0;
    if (f->ad) U.d_intra.assign(f->dfeats, f->dfeats + n_feats);
    else U.d_intra.clear();
    if (!U.tr_down.empty() || U.has_tr_mid) {
        U.tr_down.clear(); U.d_tr_down.clear(); U.has_tr_mid = false; U.tr_mid = mrisr_tensor{}; U.d_tr_mid = mrisr_tensor{};
        U.train_ws_key.clear();
    }
    mrisr_tensor x, t, e, g;
    f->describe(x, t, e, g);
    // plan OUTSIDE the capture (workspace + dry pass synchronise); a no-op while the geometry is planned
    TRY(gemm_prepare());
    if (f->ad) TRY(adapter_fit_plan(f->ad, &f->u_t, f->feats, f->dfeats, n_feats, st));
    TRY(U.train_plan(&x, &t, &e, f->ad ? f->feats : nullptr, n_feats, &g, f->loss(), st));
    char kb[128];
    snprintf(kb, sizeof(kb), ",B%d,%d,%d,L%d", f->cfg.batch, f->cfg.latent_h, f->cfg.latent_w, f->cfg.ctx_len);
    std::string key = f->model_key() + kb;
    if (f->ad) key += adapter_fit_key(f->ad);
    if (!f->exec_m || f->key_m != key) {
        TRY(capture(st, &f->exec_m, [&]() -> int {
            TRY(launch_batch(f->args(), st));
            if (f->ad) {
                TRY(launch_cond(f->cond_args(), 1, f->ai.compute_dtype, st));
                TRY(adapter_fit_forward(f->ad, &f->u_t, f->feats, n_feats, st));
            }
            TRY(U.train_step(&x, &t, &e, f->ad ? f->feats : nullptr, n_feats, &g, f->loss(), nullptr, st));
            if (f->ad) TRY(adapter_fit_backward(f->ad, f->dfeats, n_feats, st));
            hipLaunchKernelGGL(fit_micro_end_kernel, dim3(1), dim3(1), 0, st, f->ctr(), (const float*)f->loss(), f->loss_acc());
            MRISR_CHECK_HIP(hipGetLastError());
            return 0;
        }));
        f->key_m = key;
        ++f->captures;
    }
    MRISR_CHECK_HIP(hipGraphLaunch(f->exec_m, st));
    f->host_ctr[1] += 1;
    return f->leave(user, st);
    API_END
}

int mrisr_fit_apply(mrisr_fit* f, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(f, "null handle");
    MRISR_REQUIRE(f->host_ctr[0] < f->cfg.max_steps, "optimiser step past max_train_steps");
    MRISR_REQUIRE(f->host_ctr[1] == f->cfg.accum, "apply after exactly `accum` micro-batches");
    hipStream_t user = (hipStream_t)stream, st;
    TRY(f->enter(user, &st));
    Model& U = *f->m;
    const mrisr_fit_config& c = f->cfg;
    const float grad_scale = 1.0f / ((float)c.world * (float)c.accum);
    std::string key = f->model_key();
    if (f->ad) {
        char kb[160];
        snprintf(kb, sizeof(kb), ",m%p,v%p,e%p", (void*)f->ad_exp_avg, (void*)f->ad_exp_avg_sq, (void*)f->ad_ema);
        key += adapter_fit_key(f->ad) + kb;
    }
    if (f->ad && (!f->exec_o || f->key_o != key)) {
        // both buckets as one optimiser over all trainable parameters: one clip by the joint norm, one lr table, one grad_scale
        const bool lora = f->n_theta > 0;
        const AdapterFitInfo& ai = f->ai;
        const float* sched = static_cast<const float*>(f->d_sched.p);
        const float* decay = static_cast<const float*>(f->d_decay.p);
        TRY(capture(st, &f->exec_o, [&]() -> int {
            MRISR_CHECK_HIP(hipMemsetAsync(f->sumsq(), 0, sizeof(float), st));
            if (lora) TRY(launch_sumsq(U.grad, f->n_theta, f->sumsq(), st));
            TRY(launch_sumsq(ai.grad, ai.n_trainable, f->sumsq(), st));
            if (lora) {
                TRY(launch_adamw_sched(U.theta, U.grad, f->exp_avg, f->exp_avg_sq, f->n_theta, f->sumsq(), grad_scale, c.max_grad_norm,
                                       c.beta1, c.beta2, c.eps, c.weight_decay, sched, f->ctr(), c.max_steps, st));
                TRY(U.lora_refresh(st));
            }
            TRY(launch_adamw_sched(ai.theta, ai.grad, f->ad_exp_avg, f->ad_exp_avg_sq, ai.n_trainable, f->sumsq(), grad_scale,
                                   c.max_grad_norm, c.beta1, c.beta2, c.eps, c.weight_decay, sched, f->ctr(), c.max_steps, st));
            TRY(adapter_fit_repack(f->ad, st));
            if (lora && f->ema) TRY(launch_ema_sched(f->ema, U.theta, f->n_theta, decay, f->ctr(), c.max_steps, st));
            if (f->ad_ema) TRY(launch_ema_sched(f->ad_ema, ai.theta, ai.n_trainable, decay, f->ctr(), c.max_steps, st));
            hipLaunchKernelGGL(fit_step_end_kernel, dim3(1), dim3(1), 0, st, f->ctr(), f->loss_acc(), (const float*)f->sumsq(), sched,
                               1.0f / (float)c.accum, grad_scale, c.max_steps, f->loss_ring, f->gnorm_ring, f->lr_ring);
            MRISR_CHECK_HIP(hipGetLastError());
            if (lora) MRISR_CHECK_HIP(hipMemsetAsync(U.grad, 0, sizeof(float) * f->n_theta, st));
            MRISR_CHECK_HIP(hipMemsetAsync(ai.grad, 0, sizeof(float) * ai.n_trainable, st));
            return 0;
        }));
        f->key_o = key;
        ++f->captures;
    }
    if (!f->ad && (!f->exec_o || f->key_o != key)) {
        TRY(capture(st, &f->exec_o, [&]() -> int {
            MRISR_CHECK_HIP(hipMemsetAsync(f->sumsq(), 0, sizeof(float), st));
            TRY(launch_sumsq(U.grad, f->n_theta, f->sumsq(), st));
            TRY(launch_adamw_sched(U.theta, U.grad, f->exp_avg, f->exp_avg_sq, f->n_theta, f->sumsq(), grad_scale, c.max_grad_norm, c.beta1,
                                   c.beta2, c.eps, c.weight_decay, static_cast<const float*>(f->d_sched.p), f->ctr(), c.max_steps, st));
            TRY(U.lora_refresh(st));
            if (f->ema) TRY(launch_ema_sched(f->ema, U.theta, f->n_theta, static_cast<const float*>(f->d_decay.p), f->ctr(), c.max_steps, st));
            hipLaunchKernelGGL(fit_step_end_kernel, dim3(1), dim3(1), 0, st, f->ctr(), f->loss_acc(), (const float*)f->sumsq(),
                               static_cast<const float*>(f->d_sched.p), 1.0f / (float)c.accum, grad_scale, c.max_steps, f->loss_ring,
                               f->gnorm_ring, f->lr_ring);
            MRISR_CHECK_HIP(hipGetLastError());
            MRISR_CHECK_HIP(hipMemsetAsync(U.grad, 0, sizeof(float) * f->n_theta, st));
            return 0;
        }));
        f->key_o = key;
        ++f->captures;
    }
    MRISR_CHECK_HIP(hipGraphLaunch(f->exec_o, st));
    f->host_ctr[0] += 1;
    f->host_ctr[1] = 0;
    return f->leave(user, st);
    API_END
}

}  // extern "C"
