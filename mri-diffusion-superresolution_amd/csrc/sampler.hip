// The graph sampler: the fused step kernels, the host side that plans one step, captures it into a hipGraph and
// replays it, every mrisr_sampler_* entry point and the single-step test entries (mrisr_op_*_step).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "api.h"
#include "model.h"
#include "prof.h"
#include "step_plan.h"

namespace mrisr {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
static inline unsigned nblocks(long long total) {
    long long b = (total + 255) / 256;
    return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------------------------------------
// sampler steps: one fused elementwise kernel per step, coefficients from a device table indexed by a
// device-resident step counter (so one captured hipGraph replays for every step, and the reference's
// host sync on `prev_t > 0` (res_srdiff.py:92) disappears: sigma is simply 0 on the last row).
// ------------------------------------------------------------------------------------------------
// guided step (classifier-free guidance): ONE launch that combines the two halves of a [2B] UNet output,
//   e = eps_u + g (eps_c - eps_u);   phi > 0:  e *= phi std_b(eps_c) / std_b(e) + (1 - phi)   (per sample b, n-1 as torch.std),
// applies the update of the step kind (step_value, multistep_value4) to x with e, and writes the new x to the caller's latents and to both halves
// of the [2B] staging buffer the next forward reads.  eps2 rows 0..B-1 are unconditional, B..2B-1 conditional (diffusers' order).
//   phi == 0: grid-stride over float4 pieces.
//   phi  > 0: one workgroup of 1024 threads per sample; up to 16 Ki elements per sample both eps rows stay in registers (ITEMS
//             float4 pieces per thread): means, then centred sums of squares (wave shuffle -> LDS over the 16 waves), then the
//             update - eps2 is read once.  Larger samples take the re-reading kernel (three passes over eps2; correct, not fast).
// A sample whose guided prediction has no spread (centred sum of squares below f32 resolution of its mean, or per == 1) is left
// unrescaled, so an all-equal prediction cannot produce inf / NaN.
// The same kernels, templated on the number of parts K, serve the three-way step of perturbed-attention guidance with classifier-free
// guidance (K = 3): eps3 = [eps_p; eps_u; eps_c] (perturbed rows first, conditional rows last),
//   e = eps_u + g (eps_c - eps_u) + s (eps_c - eps_p),
// the same rescale, degenerate-sample guard and update, the new x to all three thirds of the staging buffer.  s == 0 is the K = 2 step.
// (PAG alone is the K = 2 step on [eps_p; eps_c] with g = 1 + s.)
// Per-step schedule: with a table `sched` [n_steps][8] the kernels read {g, s, phi} from row *step, columns 0..2,
// behind the load of *step - ordinary loads, uniform over the launch - and ignore the three launch constants; pag_alone: g := 1 + s of the
// row.  Whether the rescale kernel runs is still the host's choice (some row has phi > 0); a row with phi == 0 gives the factor
// 0 * r + 1 == 1 there, and a non-finite r is caught by the degenerate-sample guard.
// ------------------------------------------------------------------------------------------------
struct MsBuf { float* hist; float* xc; int R; };  // the multistep ring of R slabs; xc == nullptr: no corrector (DPM-Solver++)
// What one step launch reads: step_body fills it from the StepPlan, op_step from its tensors, check_step checks it and every step kernel
// takes it by value.
struct StepArgs {
    int kind = 0, K = 1;          // mrisr_step_kind; parts of the forward's output (1: unguided)
    float* x = nullptr;           // the latents [B], in place
    float* xK = nullptr;          // K > 1: the [K B] staging buffer, every part receives the new x
    const float* eps = nullptr;   // the prediction: [K B], or [B] (K == 1 and the reduced step)
    const float* lr = nullptr;    // LR anchor [B] or null
    const float* noise = nullptr; // step-noise slabs [n_steps][B] or null; slab *step is read when the row's sigma != 0
    const float* coef = nullptr;  // the coefficient table, row *step
    const int* step = nullptr;
    float clip = 0.f;
    float g = 1.f, s = 0.f, phi = 0.f;  // guidance_scale (pag alone: 1 + pag_scale), pag_scale (K == 3), guidance_rescale
    const float* sched = nullptr;       // schedule table [n][8] or null: row *step replaces the three scalars
    int sched_phi = 0, pag_alone = 0;   // some row has phi > 0 (the rescale kernel runs); K == 2 on [eps_p; eps_c], g := 1 + s of the row
    int B = 0;
    long long per = 0;            // elements per sample
    MsBuf ms{nullptr, nullptr, 0};  // multistep kinds: the history ring, UniPC's corrected state, the solver order
};
struct StepRow { float a, b, c, d, sig; };
// the three guidance scalars of this step: the launch constants, or row s of the schedule table
__device__ __forceinline__ void load_guidance(const float* sched, int s, int pag_alone, float& g, float& sp, float& phi) {
    if (!sched) return;
    const float* q = sched + 8 * (size_t)s;
    const float qs = q[1];
    g = pag_alone ? 1.f + qs : q[0];
    sp = pag_alone ? 0.f : qs;
    phi = q[2];
}
// row s of the first-order kinds' table
//   DDIM       {cx, ce}:                                                                   x = cx x + ce eps
//   Res-SRDiff {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sigma}
//   DDPM       {1/sqrt(abar_t), sqrt(1-abar_t)/sqrt(abar_t), x0 coefficient, x_t coefficient, sigma}
__device__ __forceinline__ StepRow load_step_row(int kind, const float* coef, int s) {
    StepRow r{0.f, 0.f, 0.f, 0.f, 0.f};
    if (kind > MRISR_STEP_DDPM) return r;  // multistep kinds read their own 16-float row (multistep_value4)
    if (kind == MRISR_STEP_DDIM) { r.a = coef[2 * s]; r.b = coef[2 * s + 1]; }
    else if (kind == MRISR_STEP_RESSHIFT) { r.a = coef[4 * s]; r.b = coef[4 * s + 1]; r.c = coef[4 * s + 2]; r.sig = coef[4 * s + 3]; }
    else { r.a = coef[8 * s]; r.b = coef[8 * s + 1]; r.c = coef[8 * s + 2]; r.d = coef[8 * s + 3]; r.sig = coef[8 * s + 4]; }
    return r;
}
// the update rule of the first-order kinds, one element: the only copy, for every K
__device__ __forceinline__ float step_value(int kind, const StepRow& r, float clip, float xv, float e, float l, float nz, bool noisy) {
    if (kind == MRISR_STEP_DDIM) return r.a * xv + r.b * e;
    float v;
    if (kind == MRISR_STEP_RESSHIFT) {
        const float x0 = (xv - (1.f - r.a) * l - r.b * e) / r.a;
        v = r.c * x0 + (1.f - r.c) * l;
    } else {
        float x0 = r.a * xv - r.b * e;
        if (clip > 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
        v = r.c * x0 + r.d * xv;
    }
    if (noisy) v += r.sig * nz;
    return v;
}
__device__ __forceinline__ float4 step_value4(int kind, const StepRow& r, float clip, float4 xv, float4 e, float4 l, float4 nz, bool noisy) {
    return make_float4(step_value(kind, r, clip, xv.x, e.x, l.x, nz.x, noisy), step_value(kind, r, clip, xv.y, e.y, l.y, nz.y, noisy),
                       step_value(kind, r, clip, xv.z, e.z, l.z, nz.z, noisy), step_value(kind, r, clip, xv.w, e.w, l.w, nz.w, noisy));
}
// the guided prediction of one float4 piece of a [K B] forward's output, K = 2: [eps_u; eps_c], K = 3: [eps_p; eps_u; eps_c]
//   e = eps_u + g (eps_c - eps_u)  (+ s (eps_c - eps_p), K = 3);   c = the conditional part, which the rescale rule measures against.
// Explicit fused multiply-adds: one rounding per term whatever the compiler would contract, so the K = 3 step at s == 0 has the K = 2
// step's bits.
template <int K>
__device__ __forceinline__ float4 guide4(const float* epsK, long long n, long long i, float g, float s, float4& c) {
    const float4 eu = reinterpret_cast<const float4*>(epsK + (K - 2) * n)[i];
    c = reinterpret_cast<const float4*>(epsK + (K - 1) * n)[i];
    const float4 e = make_float4(fmaf(g, c.x - eu.x, eu.x), fmaf(g, c.y - eu.y, eu.y), fmaf(g, c.z - eu.z, eu.z), fmaf(g, c.w - eu.w, eu.w));
    if (K == 2) return e;
    const float4 ep = reinterpret_cast<const float4*>(epsK)[i];
    return make_float4(fmaf(s, c.x - ep.x, e.x), fmaf(s, c.y - ep.y, e.y), fmaf(s, c.z - ep.z, e.z), fmaf(s, c.w - ep.w, e.w));
}
__device__ __forceinline__ float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ssq4(float4 v, float m) {
    const float a = v.x - m, b = v.y - m, c = v.z - m, d = v.w - m;
    return (a * a + b * b) + (c * c + d * d);
}
__device__ __forceinline__ float4 scale4(float4 v, float f) { return make_float4(v.x * f, v.y * f, v.z * f, v.w * f); }
// one float4 piece to x and to every part of the [K B] staging buffer
template <int K>
__device__ __forceinline__ void store_parts(float* x, float* xK, long long n, long long i4, float4 v) {
    reinterpret_cast<float4*>(x)[i4] = v;
#pragma unroll
    for (int k = 0; k < K; ++k) reinterpret_cast<float4*>(xK + k * n)[i4] = v;
}

// ------------------------------------------------------------------------------------------------
// multistep step (UniPC bh2 / DPM-Solver++ 2M, data prediction): ONE launch per step.  Every quantity of a linear multistep
// step is linear in (z, eps, previous corrected state, history), z = x - LR (LR-anchored run) or x, so the host folds the order
// schedule, the cold first step, disabled correctors and the final point into one row of 16 floats per step
// (build_multistep_rows below); a zero coefficient switches an absent term off and nothing here branches on the step:
//   row = { m: z, eps | corrected state: z, eps, xc, h1, h2, h3 | next state: z, eps, xc, h1, h2, h3 | 0, 0 }
//   m   = the x0 prediction at this step            -> history slot s % R   (h_k = the prediction k steps back, slot (s - k) % R)
//   zc  = the corrected state (UniPC; else unused)  -> xc
//   x   = next state + LR
// The three forms are folded separately down to the raw inputs, so the next state never goes through the ill-conditioned
// m = (z - sigma eps) / alpha of a high-noise step, and order 1 is the DDIM expression itself.  R = solver_order slabs of n floats;
// the slot an element overwrites is the one it read as h_R.  The ring and xc are zeroed by the host at the start of a run.
// ------------------------------------------------------------------------------------------------
constexpr int MS_ROW = 16;
__device__ __forceinline__ float4 fma4(float c, float4 v, float4 acc) {
    return make_float4(fmaf(c, v.x, acc.x), fmaf(c, v.y, acc.y), fmaf(c, v.z, acc.z), fmaf(c, v.w, acc.w));
}
// one float4 piece: reads the history and xc, writes history slot s % R and xc, returns the new x
__device__ __forceinline__ float4 multistep_value4(const float* __restrict__ row, const MsBuf& ms, int s, long long n, long long i,
                                                   float4 xv, float4 e, float4 l) {
    const float4 z = make_float4(xv.x - l.x, xv.y - l.y, xv.z - l.z, xv.w - l.w);
    const int cur = s % ms.R;
    float4 m = fma4(row[1], e, scale4(z, row[0]));
    float4 zc = fma4(row[3], e, scale4(z, row[2]));
    float4 zn = fma4(row[9], e, scale4(z, row[8]));
    if (ms.xc) {
        const float4 xc = reinterpret_cast<const float4*>(ms.xc)[i];
        zc = fma4(row[4], xc, zc);
        zn = fma4(row[10], xc, zn);
    }
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
        if (k <= ms.R) {
            const int slot = (cur + ms.R - (k % ms.R)) % ms.R;
            const float4 h = reinterpret_cast<const float4*>(ms.hist + (size_t)slot * n)[i];
            zc = fma4(row[4 + k], h, zc);
            zn = fma4(row[10 + k], h, zn);
        }
    }
    reinterpret_cast<float4*>(ms.hist + (size_t)cur * n)[i] = m;
    if (ms.xc) reinterpret_cast<float4*>(ms.xc)[i] = zc;
    return make_float4(zn.x + l.x, zn.y + l.y, zn.z + l.z, zn.w + l.w);
}
// what every step kernel derives from its StepArgs behind the load of *step, uniform over the launch
struct StepCtx {
    int s;
    long long n;         // B * per
    StepRow r;
    const float* msrow;  // the multistep kinds' row, or null
    const float* noise;  // this step's slab [n], or null: no noise given, or a row with sigma == 0
};
__device__ __forceinline__ StepCtx load_step_ctx(const StepArgs& a) {
    StepCtx c;
    c.s = *a.step;
    c.n = (long long)a.B * a.per;
    c.r = load_step_row(a.kind, a.coef, c.s);
    c.msrow = a.ms.hist ? a.coef + (size_t)MS_ROW * c.s : nullptr;
    c.noise = a.noise && c.r.sig != 0.f ? a.noise + (size_t)c.s * c.n : nullptr;
    return c;
}
// the update of one float4 piece from the prediction e: the first-order kinds, or the multistep step; the new x goes to the caller's
// latents and to PARTS parts of the staging buffer
template <int PARTS>
__device__ __forceinline__ void guided_apply4(const StepArgs& a, const StepCtx& c, long long i, float4 e) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
    const float4 l = a.lr ? reinterpret_cast<const float4*>(a.lr)[i] : z4;
    float4 v;
    if (c.msrow) {
        v = multistep_value4(c.msrow, a.ms, c.s, c.n, i, xv, e, l);
    } else {
        const float4 nz = c.noise ? reinterpret_cast<const float4*>(c.noise)[i] : z4;
        v = step_value4(a.kind, c.r, a.clip, xv, e, l, nz, c.noise != nullptr);
    }
    store_parts<PARTS>(a.x, a.xK, c.n, i, v);
}
// The plain first-order step (K = 1; DDIM / Res-SRDiff / DDPM): scalar and grid-stride over n, so an unguided run has no multiple-of-4
// or alignment precondition.
__global__ void plain_step_kernel(StepArgs a) {
    const StepCtx c = load_step_ctx(a);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < c.n; i += (long long)gridDim.x * 256)
        a.x[i] = step_value(a.kind, c.r, a.clip, a.x[i], a.eps[i], a.lr ? a.lr[i] : 0.f, c.noise ? c.noise[i] : 0.f, c.noise != nullptr);
}
// The update from a single prediction eps [B], any step kind, float4 pieces, grid-stride.  PARTS = 0: the plain multistep step (K = 1).
// PARTS = 2 / 3: the reduced step of a guided / pag run whose schedule row is neutral (g == 1, s == 0).  The guided
// prediction of such a row is the conditional one, whatever phi (a prediction rescaled against itself: factor 1), so the forward ran on the
// conditional rows alone and eps is their prediction - the last part of the run's [K B] output buffer.  The history ring and UniPC's
// corrected state are written exactly as a guided step writes them, and the new x goes to ALL K parts of the staging buffer: the next
// guided step finds every part current.
template <int PARTS>
__global__ __launch_bounds__(256) void single_step_kernel(StepArgs a) {
    const StepCtx c = load_step_ctx(a);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < (c.n >> 2); i += (long long)gridDim.x * 256)
        guided_apply4<PARTS>(a, c, i, reinterpret_cast<const float4*>(a.eps)[i]);
}
constexpr int GS_THREADS = 1024;
// sums of (a, b) over the workgroup, the same value in every thread; `red` holds one pair per wave
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
    a = wsum(a);
    b = wsum(b);
    __syncthreads();  // the previous round's readers are done with `red`
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = a; red[2 * (threadIdx.x >> 6) + 1] = b; }
    __syncthreads();
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int w = 0; w < GS_THREADS / 64; ++w) { sa += red[2 * w]; sb += red[2 * w + 1]; }
    a = sa;
    b = sb;
}
// phi std(eps_c) / std(e) + (1 - phi) from the centred sums of squares (the n-1 of both estimates cancels)
__device__ __forceinline__ float rescale_factor(float qc, float qe, float me, int per, float phi) {
    if (per < 2 || !(qe > 1e-12f * (float)per * me * me) || !(qe > 0.f)) return 1.f;
    const float f = phi * sqrtf(qc / qe) + (1.f - phi);
    return f <= 3.0e38f ? f : 1.f;
}

template <int K>
__global__ __launch_bounds__(256) void guided_step_kernel(StepArgs a) {
    const StepCtx c = load_step_ctx(a);
    float g = a.g, sp = a.s, phi = 0.f;  // phi is not read here
    load_guidance(a.sched, c.s, a.pag_alone, g, sp, phi);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < (c.n >> 2); i += (long long)gridDim.x * 256) {
        float4 cc;
        const float4 e = guide4<K>(a.eps, c.n, i, g, sp, cc);
        guided_apply4<K>(a, c, i, e);
    }
}

template <int K, int ITEMS>
__global__ __launch_bounds__(GS_THREADS) void guided_step_rescale_kernel(StepArgs a) {
    __shared__ float red[2 * GS_THREADS / 64];
    const StepCtx cx = load_step_ctx(a);
    float g = a.g, sp = a.s, phi = a.phi;
    load_guidance(a.sched, cx.s, a.pag_alone, g, sp, phi);
    const int per = (int)a.per, per4 = per >> 2;
    const long long base4 = (long long)blockIdx.x * per4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 e[ITEMS], c[ITEMS];
    float sc = 0.f, se = 0.f;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int j = threadIdx.x + k * GS_THREADS;
        e[k] = z4; c[k] = z4;
        if (j < per4) {
            e[k] = guide4<K>(a.eps, cx.n, base4 + j, g, sp, c[k]);
            sc += sum4(c[k]); se += sum4(e[k]);
        }
    }
    block_sum2(sc, se, red);
    const float mc = sc / (float)per, me = se / (float)per;
    float qc = 0.f, qe = 0.f;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k)
        if (threadIdx.x + k * GS_THREADS < per4) { qc += ssq4(c[k], mc); qe += ssq4(e[k], me); }
    block_sum2(qc, qe, red);
    const float f = rescale_factor(qc, qe, me, per, phi);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int j = threadIdx.x + k * GS_THREADS;
        if (j < per4) guided_apply4<K>(a, cx, base4 + j, scale4(e[k], f));
    }
}
// samples too large for the register file: the same three passes, each re-reading eps
template <int K>
__global__ __launch_bounds__(GS_THREADS) void guided_step_rescale_reread_kernel(StepArgs a) {
    __shared__ float red[2 * GS_THREADS / 64];
    const StepCtx cx = load_step_ctx(a);
    float g = a.g, sp = a.s, phi = a.phi;
    load_guidance(a.sched, cx.s, a.pag_alone, g, sp, phi);
    const int per = (int)a.per, per4 = per >> 2;
    const long long base4 = (long long)blockIdx.x * per4;
    float4 c;
    float sc = 0.f, se = 0.f;
    for (int j = threadIdx.x; j < per4; j += GS_THREADS) { const float4 e = guide4<K>(a.eps, cx.n, base4 + j, g, sp, c); sc += sum4(c); se += sum4(e); }
    block_sum2(sc, se, red);
    const float mc = sc / (float)per, me = se / (float)per;
    float qc = 0.f, qe = 0.f;
    for (int j = threadIdx.x; j < per4; j += GS_THREADS) { const float4 e = guide4<K>(a.eps, cx.n, base4 + j, g, sp, c); qc += ssq4(c, mc); qe += ssq4(e, me); }
    block_sum2(qc, qe, red);
    const float f = rescale_factor(qc, qe, me, per, phi);
    for (int j = threadIdx.x; j < per4; j += GS_THREADS)
        guided_apply4<K>(a, cx, base4 + j, scale4(guide4<K>(a.eps, cx.n, base4 + j, g, sp, c), f));
}

template <int K>
static void launch_guided_kernels(const StepArgs& a, hipStream_t st) {
    const long long n = (long long)a.B * a.per;
    if (a.sched ? !a.sched_phi : a.phi == 0.f) {
        hipLaunchKernelGGL(guided_step_kernel<K>, dim3(nblocks(n >> 2)), dim3(256), 0, st, a);
        return;
    }
    if (a.per <= 4 * GS_THREADS) hipLaunchKernelGGL((guided_step_rescale_kernel<K, 1>), dim3(a.B), dim3(GS_THREADS), 0, st, a);
    else if (a.per <= 8 * GS_THREADS) hipLaunchKernelGGL((guided_step_rescale_kernel<K, 2>), dim3(a.B), dim3(GS_THREADS), 0, st, a);
    else if (a.per <= 16 * GS_THREADS) hipLaunchKernelGGL((guided_step_rescale_kernel<K, 4>), dim3(a.B), dim3(GS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(guided_step_rescale_reread_kernel<K>, dim3(a.B), dim3(GS_THREADS), 0, st, a);
}
// The operand checks of every step launch, once.  who: the message prefix of the launch - "guided step: " (K = 2), "pag step: " (K = 3),
// "reduced step: ", "multistep step: " (K = 1; the plain first-order launch, which has nothing but null operands to check: "step: ").  Also drops what this kind does not read (lr, noise, the ring, xc), so the kernels and the
// byte count below see null for it.
static int check_step(const std::string& who, StepArgs& a, bool reduced) {
    MRISR_REQUIRE(a.K == 2 || a.K == 3 || (a.K == 1 && !reduced), who + "2 or 3 parts");
    MRISR_REQUIRE(a.kind >= MRISR_STEP_DDIM && a.kind <= MRISR_STEP_DPMSOLVERPP, who + "unknown step kind");
    const bool multistep = a.kind > MRISR_STEP_DDPM, guided = a.K > 1 && !reduced;
    const long long n = (long long)a.B * a.per;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    float* const xc = a.ms.xc;
    a.ms = MsBuf{multistep ? a.ms.hist : nullptr, multistep && a.kind == MRISR_STEP_UNIPC ? xc : nullptr, multistep ? a.ms.R : 0};
    if (multistep) {
        MRISR_REQUIRE(a.x && a.eps && a.ms.hist && a.ms.R >= 1 && a.ms.R <= 3, "multistep step: null operand or solver order outside 1..3");
        MRISR_REQUIRE(n > 0 && n % 4 == 0, "multistep step: C*h*w of the latents must be a multiple of 4");
        MRISR_REQUIRE(al16(a.x) && al16(a.eps) && al16(a.lr) && al16(a.ms.hist) && al16(a.ms.xc), "multistep step: operands must be 16-byte aligned");
        MRISR_REQUIRE(a.kind != MRISR_STEP_UNIPC || xc, who + "UniPC needs the corrected-state buffer");
    }
    MRISR_REQUIRE(a.x && a.eps && a.coef && a.step && (a.K == 1 || (a.xK && a.B > 0 && a.per > 0)), who + "null operand");
    if (a.K > 1) MRISR_REQUIRE(a.per % 4 == 0 && a.per < (1ll << 31), who + "the per-sample size must be a multiple of 4");
    if (guided && a.sched) {  // the three scalars are not read: the rows were checked when the table was built
        MRISR_REQUIRE(!a.pag_alone || a.K == 2, who + "pag alone is the step on 2 parts");
        MRISR_REQUIRE((reinterpret_cast<uintptr_t>(a.sched) & 3) == 0, who + "the schedule table must be 4-byte aligned");
    } else if (guided) {
        MRISR_REQUIRE(a.phi >= 0.f && a.phi <= 1.f, who + "guidance_rescale must lie in [0, 1]");
        if (a.K == 3) MRISR_REQUIRE(std::isfinite(a.s) && a.s >= 0.f, who + "pag_scale must be finite and >= 0");
    }
    MRISR_REQUIRE(a.kind != MRISR_STEP_RESSHIFT || a.lr, who + "Res-SRDiff needs the LR anchor latents");
    if (a.K > 1) MRISR_REQUIRE(al16(a.x) && al16(a.xK) && al16(a.eps) && al16(a.lr) && al16(a.noise), who + "operands must be 16-byte aligned");
    if (a.kind != MRISR_STEP_RESSHIFT && !multistep) a.lr = nullptr;
    if (a.kind == MRISR_STEP_DDIM || multistep) a.noise = nullptr;
    return 0;
}
// ONE launch: the guided step of a [K B] prediction (K = 2, 3), the reduced step of a guided / pag run from the conditional prediction
// [B], or the unguided step (K = 1)
static int launch_step(StepArgs a, bool reduced, hipStream_t st) {
    const bool multistep = a.kind > MRISR_STEP_DDPM, guided = a.K > 1 && !reduced;
    const char* who = reduced ? "reduced step: " : a.K == 3 ? "pag step: " : a.K != 1 ? "guided step: " : multistep ? "multistep step: " : "step: ";
    if (int rc = check_step(who, a, reduced)) return rc;
    const long long n = (long long)a.B * a.per;
    // eps (a guided step: K times), x in, 1 + K stores of x (K = 1: one), lr; the plain first-order step of a stochastic kind: + its noise
    // slab; multistep: + `order` history reads, one history write, xc in and out
    double bytes = guided ? (a.K == 3 ? 32.0 : 28.0) : 12.0 + (a.K > 1 ? 4.0 * a.K : 0.0);
    bytes += (a.lr ? 4.0 : 0.0) + (multistep ? 4.0 * a.ms.R + 4.0 + (a.ms.xc ? 8.0 : 0.0) : 0.0);
    if (a.K == 1 && (a.kind == MRISR_STEP_RESSHIFT || a.kind == MRISR_STEP_DDPM)) bytes += 4.0;
    ProfScope ps("sampler_step", 0.0, bytes * n, st);
    if (guided && a.K == 3) launch_guided_kernels<3>(a, st);
    else if (guided) launch_guided_kernels<2>(a, st);
    else if (a.K == 3) hipLaunchKernelGGL(single_step_kernel<3>, dim3(nblocks(n >> 2)), dim3(256), 0, st, a);
    else if (a.K == 2) hipLaunchKernelGGL(single_step_kernel<2>, dim3(nblocks(n >> 2)), dim3(256), 0, st, a);
    else if (multistep) hipLaunchKernelGGL(single_step_kernel<0>, dim3(nblocks(n >> 2)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(plain_step_kernel, dim3(nblocks(n)), dim3(256), 0, st, a);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ void advance_step_kernel(int* step) { *step += 1; }
static int launch_advance_step(int* step_idx, hipStream_t st) {
    hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(1), 0, st, step_idx);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
__global__ void resshift_forward_kernel(const float* hr, const float* lr, const float* noise, const float* ac,
                                        const long long* t, int t_is_scalar, float* out, int B, long long per) {
    const long long n = (long long)B * per;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / per);
        const float a = ac[t_is_scalar ? t[0] : t[b]];
        const float ra = sqrtf(a);
        out[i] = ra * hr[i] + (1.f - ra) * lr[i] + sqrtf(1.f - a) * noise[i];
    }
}
int launch_resshift_forward(const float* hr, const float* lr, const float* noise, const float* alphas_cumprod,
                            const long long* t, int t_is_scalar, float* out, int B, long long per_sample,
                            hipStream_t st) {
    hipLaunchKernelGGL(resshift_forward_kernel, dim3(nblocks((long long)B * per_sample)), dim3(256), 0, st, hr, lr,
                       noise, alphas_cumprod, t, t_is_scalar, out, B, per_sample);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// the checks a schedule table passes before anything touches the device: 0, or the error code with the message set
int check_schedule_rows(const float* rows, int n_rows) {
    static const char* const names[8] = {"guidance_scale (g)", "pag_scale (s)", "guidance_rescale (phi)", "freeu_s1", "freeu_s2", "freeu_b1", "freeu_b2", "the padding column"};
    for (int i = 0; i < n_rows; ++i) {
        const float* r = rows + 8 * (size_t)i;
        for (int c = 0; c < 8; ++c)
            MRISR_REQUIRE(std::isfinite(r[c]), "schedule: row " + std::to_string(i) + ": " + names[c] + " is not finite");
        MRISR_REQUIRE(r[1] >= 0.f, "schedule: row " + std::to_string(i) + ": pag_scale (s) must be >= 0");
        MRISR_REQUIRE(r[2] >= 0.f && r[2] <= 1.f, "schedule: row " + std::to_string(i) + ": guidance_rescale (phi) must lie in [0, 1]");
        for (int c = 3; c < 7; ++c) MRISR_REQUIRE(r[c] >= 0.f, "schedule: row " + std::to_string(i) + ": " + names[c] + " must be >= 0");
    }
    return 0;
}

}  // namespace mrisr

// =================================================================================================
// host side: the sampler handle, its setters, the run
// =================================================================================================
using namespace mrisr;

struct mrisr_model : public Model {};

__global__ void load_t_kernel(long long* cur_t, const long long* table, const int* step) { *cur_t = table[*step]; }

static int g_temb_table = -1;  // test hook: -1 = MRISR_TEMB_TABLE (default 1), 0 off, 1 on
extern "C" void mrisr_debug_temb_table(int on) { g_temb_table = on; }
static bool temb_table_enabled() {
    static const int env = [] { const char* e = getenv("MRISR_TEMB_TABLE"); return e ? atoi(e) : 1; }();
    return g_temb_table < 0 ? env != 0 : g_temb_table != 0;
}
// ---- multistep solvers (UniPC bh2 / DPM-Solver++ 2M): one row of 16 folded coefficients per step (layout: multistep_value4 above) ----
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

// A per-step table of a sampler (the schedule, [n_steps][8]; the conditioning strengths, [n_steps][4]): the host rows (empty: no table)
// and the device buffer every run with a table uploads them to - reserved once, so its address is the same for every such run.
struct StepTable {
    const char* name;
    int width;
    std::vector<float> rows;
    DevBuf dev;
    bool on() const { return !rows.empty(); }
    const float* row(int i) const { return &rows[(size_t)width * i]; }
    // NULL / 0 clears the table (the next run has another plan and captures again); otherwise n_steps rows that pass `check`
    int set(const float* rows_host, int n_rows, int n_steps, int (*check)(const float*, int)) {
        const std::string who = std::string(name) + ": ";
        if (!rows_host || n_rows == 0) {
            MRISR_REQUIRE(!rows_host && n_rows == 0, who + "NULL / 0 clears it; rows need n_rows == n_steps");
            rows.clear();
            return 0;
        }
        MRISR_REQUIRE(n_rows == n_steps, who + "n_rows must equal the sampler's n_steps (" + std::to_string(n_steps) + "), got " + std::to_string(n_rows));
        if (int rc = check(rows_host, n_rows)) return rc;
        TRY(dev.reserve(sizeof(float) * width * (size_t)n_steps, false));  // once per sampler: n_rows is always n_steps
        rows.assign(rows_host, rows_host + (size_t)width * n_rows);
        return 0;
    }
    // The rows, indexed by the absolute step like the coefficient rows.  `rows` is pageable and may be replaced (set) right after the run
    // returns: this relies on the runtime staging a pageable host-to-device copy before hipMemcpyAsync returns.
    int upload(int n_steps, hipStream_t st) {
        MRISR_REQUIRE(rows.size() == (size_t)width * n_steps && dev.bytes >= sizeof(float) * rows.size(), std::string(name) + " table size");
        MRISR_CHECK_HIP(hipMemcpyAsync(dev.p, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, st));
        return 0;
    }
};

struct mrisr_sampler {
    mrisr_model* unet = nullptr;
    mrisr_model* cnet = nullptr;
    int kind = 0, n_steps = 0, first = 0, last = 0;
    float clip = 0.f;
    float guidance_scale = 1.f, guidance_rescale = 0.f;  // classifier-free guidance of mrisr_sampler_run_guided
    unsigned pag_mask = 0;  // perturbed-attention guidance of mrisr_sampler_run_pag: the applied transformer blocks and the scale
    float pag_scale = 0.f;
    int n_captures = 0;     // step graphs captured so far (mrisr_sampler_num_captures)
    // per-step schedule (mrisr_sampler_set_schedule): rows of 8 (no table: the scalars above rule), and what the
    // checks and the kernel choice need of the values: some row with phi > 0 / s > 0 / g != 1 / FreeU columns other than 1
    StepTable sched{"schedule", 8};
    bool sched_phi = false, sched_s = false, sched_g = false, sched_freeu = false;
    // conditioning strength (mrisr_sampler_set_conditioning): rows {c, a, 0, 0} (no table: every residual and feature
    // at full strength, added as before), and what the checks need of the values: some row with c != 1 / a != 1
    StepTable cond{"conditioning", 4};
    bool cond_guess = false, cond_c = false, cond_a = false;
    // low-frequency consistency (mrisr_sampler_set_consistency): rows {w, alpha, beta, sigma} (no table: no launch), the
    // launch constants, and the caller's reference [B, C, h, w] and noise slabs [n_steps][B, C, h, w] (or null), remembered for the runs
    StepTable cons{"consistency", 4};
    int cons_factor = 0, cons_filter = 0;
    const float* cons_ref = nullptr;
    const float* cons_noise = nullptr;
    long long cons_shape[4] = {0, 0, 0, 0};
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
    // shallow (reads it) otherwise; interval 1 = no cache: the body, the plan and the graph without it
    int cache_interval = 1, cache_depth = 1;
    DevBuf d_cache;
    // tiled sampling: tile_h == 0 is off.  A run whose grid has more than one tile gathers the state into d_xt
    // [NB*T, C, t_h, t_w], runs the forward there into d_et and blends d_et into d_eps; the grid and the window tables live in d_tiles
    int tile_h = 0, tile_w = 0, tile_oh = 0, tile_ow = 0, tile_window = MRISR_TILE_GAUSSIAN;
    TilePlan tiles;
    DevBuf d_tiles, d_xt, d_et;
    // skipping (mrisr_sampler_set_skip): each step runs only the rows and networks its table rows need.  variant[i] of
    // the last run: the STEP_* bits of step i (all zero with the option off); stats: what mrisr_sampler_run_stats reports
    bool skip = false;
    std::vector<unsigned char> variant;
    long long stats[4] = {0, 0, 0, 0};
    // one graph per step variant, each captured the first time a run needs it; exec[0] is the full step (cache_interval > 1: full + store)
    hipGraphExec_t exec[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipGraphExec_t exec_shallow = nullptr;  // cache_interval > 1: the shallow step
    StepPlan plan = new_step_plan();        // what every graph above was captured from
    void drop_graphs() {
        for (hipGraphExec_t& e : exec) {
            if (e) (void)hipGraphExecDestroy(e);
            e = nullptr;
        }
        if (exec_shallow) (void)hipGraphExecDestroy(exec_shallow);
        exec_shallow = nullptr;
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

// The options of a sampler that exclude each other.  current_options reads them off the sampler as it stands: no pag run, no conditioning
// table, which belong to a run.  A setter overrides the one field it is about to set, the run fills in its own three.
struct Options {
    bool has_cnet;
    int cache_interval;
    bool tiles_on;
    bool pag_run;
    bool cond_table, guess;  // the conditioning table and guess mode of the run
    bool skip;               // the skipping of neutral steps (mrisr_sampler_set_skip)
    bool cons_table;         // the consistency table (mrisr_sampler_set_consistency)
};
static Options current_options(const mrisr_sampler* s) {
    return Options{s->cnet != nullptr, s->cache_interval, s->tile_h != 0, false, false, false, s->skip, s->cons.on()};
}
// Every rule once: the first one that the UNet's state and `o` violate, or null.  Always asked before any launch.
static const char* option_conflict(const Model& U, const Options& o) {
    const bool cached = o.cache_interval > 1;
    if (o.skip && cached) return "skipping neutral steps together with a feature cache (interval > 1) is not supported";
    if (o.cond_table && cached) return "conditioning: a conditioning table together with a feature cache (interval > 1) is not supported";
    if (o.cons_table && cached) return "consistency: a consistency table together with a feature cache (interval > 1) is not supported";
    if (o.guess && o.pag_run) return "conditioning: guess mode in a pag run is not supported";
    if (o.guess && o.tiles_on) return "conditioning: guess mode together with tiles is not supported";
    if (o.cond_table && U.keep) return "conditioning: a training forward is being recorded";
    if (cached && o.has_cnet) return "a feature cache (interval > 1) together with a ControlNet is not supported";
    if (cached && o.tiles_on) return "a feature cache (interval > 1) together with tiles is not supported";
    if (cached && U.freeu.on) return "a feature cache (interval > 1) together with FreeU is not supported (mrisr_model_set_freeu)";
    if (cached && o.pag_run) return "pag run: a feature cache with interval > 1 is not supported (the shallow pass skips the blocks pag perturbs)";
    if (o.pag_run && U.cfg.fp8_attention) return "pag run: not supported on a UNet built with fp8_attention";
    if (o.pag_run && U.keep) return "pag run: a training forward is being recorded";
    if (U.freeu.on && U.keep) return "FreeU: a training forward is being recorded";
    return nullptr;
}

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
    Options o = current_options(s);
    o.cache_interval = interval;
    const char* conflict = option_conflict(*s->unet, o);
    MRISR_REQUIRE(!conflict, conflict);
    if (interval != s->cache_interval || depth != s->cache_depth) s->drop_graphs();  // the next run captures again
    s->cache_interval = interval;
    s->cache_depth = depth;
    return 0;
}

int mrisr_sampler_set_tiles(mrisr_sampler* s, int tile_h, int tile_w, int overlap_h, int overlap_w, int window) {
    MRISR_REQUIRE(s, "null sampler");
    if (tile_h == 0) {  // off: the body, the plan and the graph without tiles
        if (s->tile_h) s->drop_graphs();
        s->tile_h = s->tile_w = s->tile_oh = s->tile_ow = 0;
        return 0;
    }
    const int d = 1 << (s->unet->cfg.num_levels - 1);  // the UNet's own divisibility rule for h and w
    MRISR_REQUIRE(tile_h >= d && tile_w >= d && tile_h % d == 0 && tile_w % d == 0, "tile: a multiple of 2^(num_levels-1), at least that");
    MRISR_REQUIRE(overlap_h >= 0 && overlap_w >= 0 && overlap_h < tile_h && overlap_w < tile_w && overlap_h % d == 0 && overlap_w % d == 0,
                  "overlap: a multiple of 2^(num_levels-1) in 0 .. tile - 1");
    MRISR_REQUIRE(window == MRISR_TILE_UNIFORM || window == MRISR_TILE_GAUSSIAN, "window: MRISR_TILE_UNIFORM or MRISR_TILE_GAUSSIAN");
    Options o = current_options(s);
    o.tiles_on = true;
    const char* conflict = option_conflict(*s->unet, o);
    MRISR_REQUIRE(!conflict, conflict);
    if (tile_h != s->tile_h || tile_w != s->tile_w || overlap_h != s->tile_oh || overlap_w != s->tile_ow || window != s->tile_window)
        s->drop_graphs();
    s->tile_h = tile_h; s->tile_w = tile_w; s->tile_oh = overlap_h; s->tile_ow = overlap_w; s->tile_window = window;
    return 0;
}

int mrisr_sampler_set_guidance(mrisr_sampler* s, float guidance_scale, float guidance_rescale) {
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(std::isfinite(guidance_scale), "guidance_scale must be finite");
    MRISR_REQUIRE(guidance_rescale >= 0.f && guidance_rescale <= 1.f, "guidance_rescale must lie in [0, 1]");
    s->guidance_scale = guidance_scale;  // passed to the step kernel by value: part of the step plan
    s->guidance_rescale = guidance_rescale;
    return 0;
}

int mrisr_sampler_set_pag(mrisr_sampler* s, unsigned block_mask, float pag_scale) {
    MRISR_REQUIRE(s, "null sampler");
    MRISR_REQUIRE(std::isfinite(pag_scale) && pag_scale >= 0.f, "pag_scale must be finite and >= 0");
    const int nb = s->unet->num_transformer_blocks();
    MRISR_REQUIRE(nb >= 32 || (block_mask >> nb) == 0, "pag: block_mask selects blocks the UNet does not have (mrisr_model_num_transformer_blocks)");
    MRISR_REQUIRE(pag_scale == 0.f || block_mask != 0, "pag: pag_scale > 0 needs at least one applied block in block_mask");
    s->pag_mask = block_mask;  // both are part of the step plan of the next mrisr_sampler_run_pag
    s->pag_scale = pag_scale;
    return 0;
}
int mrisr_sampler_num_captures(const mrisr_sampler* s) { return s ? s->n_captures : 0; }

// Skipping: with `on`, each step of the next runs forwards only the rows and networks its table rows need
// (step_variant below).  Off (the default): every step is the full one - the launches, bits and captures of a sampler that never had it.
// The variants share one step plan, so neither value drops a graph.
int mrisr_sampler_set_skip(mrisr_sampler* s, int on) {
    MRISR_REQUIRE(s, "null sampler");
    Options o = current_options(s);
    o.skip = on != 0;
    const char* conflict = option_conflict(*s->unet, o);
    MRISR_REQUIRE(!conflict, conflict);
    s->skip = on != 0;
    return 0;
}
// the last run: {sum over its steps of the UNet forward's rows, steps that ran the ControlNet, steps that took adapter features, distinct
// step variants}
int mrisr_sampler_run_stats(const mrisr_sampler* s, int64_t out[4]) {
    MRISR_REQUIRE(s && out, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = s->stats[k];
    return 0;
}

int mrisr_sampler_set_schedule(mrisr_sampler* s, const float* rows_host, int n_rows) {
    API_BEGIN
    MRISR_REQUIRE(s, "null sampler");
    TRY(s->sched.set(rows_host, n_rows, s->n_steps, check_schedule_rows));
    s->sched_phi = s->sched_s = s->sched_g = s->sched_freeu = false;
    for (int i = 0; i < s->n_steps && s->sched.on(); ++i) {
        const float* r = s->sched.row(i);
        s->sched_g |= r[0] != 1.f;
        s->sched_s |= r[1] > 0.f;
        s->sched_phi |= r[2] > 0.f;
        s->sched_freeu |= r[3] != 1.f || r[4] != 1.f || r[5] != 1.f || r[6] != 1.f;
    }
    return 0;
    API_END
}

int mrisr_sampler_set_conditioning(mrisr_sampler* s, const float* rows_host, int n_rows, int guess_mode) {
    API_BEGIN
    MRISR_REQUIRE(s, "null sampler");
    TRY(s->cond.set(rows_host, n_rows, s->n_steps, check_conditioning_rows));
    s->cond_guess = s->cond.on() && guess_mode != 0;
    s->cond_c = s->cond_a = false;
    for (int i = 0; i < s->n_steps && s->cond.on(); ++i) {
        s->cond_c |= s->cond.row(i)[0] != 1.f;
        s->cond_a |= s->cond.row(i)[1] != 1.f;
    }
    return 0;
    API_END
}

int mrisr_sampler_set_consistency(mrisr_sampler* s, int factor, int filter, const float* rows_host, int n_rows, const mrisr_tensor* ref,
                                  const mrisr_tensor* noise) {
    API_BEGIN
    MRISR_REQUIRE(s, "null sampler");
    if (!rows_host || n_rows == 0) {  // clears everything: the next run has another plan and captures again
        TRY(s->cons.set(rows_host, n_rows, s->n_steps, check_consistency_rows));
        s->cons_factor = s->cons_filter = 0;
        s->cons_ref = s->cons_noise = nullptr;
        return 0;
    }
    MRISR_REQUIRE(n_rows == s->n_steps, "consistency: n_rows must equal the sampler's n_steps (" + std::to_string(s->n_steps) + "), got " + std::to_string(n_rows));
    TRY(check_consistency_rows(rows_host, n_rows));
    MRISR_REQUIRE(ref && ref->data && ref->ndim == 4 && ref->dtype == MRISR_F32 && ref->layout == MRISR_NCHW, "consistency: ref must be f32 [B, C, h, w]");
    MRISR_REQUIRE(ref->shape[0] > 0 && ref->shape[1] == s->unet->cfg.in_channels && ref->shape[2] > 0 && ref->shape[3] > 0 &&
                      ref->shape[2] < (1 << 20) && ref->shape[3] < (1 << 20),
                  "consistency: ref must have the latents' shape [B, in_channels, h, w]");
    TRY(check_consistency_geometry(factor, filter, (int)ref->shape[2], (int)ref->shape[3]));
    bool noisy = false;
    for (int i = 0; i < n_rows; ++i) noisy |= rows_host[4 * (size_t)i + 3] != 0.f;
    MRISR_REQUIRE(noise || !noisy, "consistency: rows with sigma != 0 need the noise slabs");
    if (noise) {
        long long k = 1, per = 1;
        for (int i = 0; i < noise->ndim; ++i) k *= noise->shape[i];
        for (int i = 0; i < 4; ++i) per *= ref->shape[i];
        MRISR_REQUIRE(noise->data && noise->dtype == MRISR_F32 && k == (long long)s->n_steps * per,
                      "consistency: noise must be f32 [n_steps, B, C, h, w] with the shape of ref");
    }
    Options o = current_options(s);
    o.cons_table = true;
    const char* conflict = option_conflict(*s->unet, o);
    MRISR_REQUIRE(!conflict, conflict);
    TRY(s->cons.set(rows_host, n_rows, s->n_steps, check_consistency_rows));
    s->cons_factor = factor; s->cons_filter = filter;
    s->cons_ref = static_cast<const float*>(ref->data);
    s->cons_noise = noise ? static_cast<const float*>(noise->data) : nullptr;
    for (int i = 0; i < 4; ++i) s->cons_shape[i] = ref->shape[i];
    return 0;
    API_END
}

}  // extern "C"

// ---- one run: mrisr_sampler_run (K = 1: B rows everywhere), mrisr_sampler_run_guided (K = 2) and mrisr_sampler_run_pag (pag: K = 2 or 3).
// The forwards see NB = K B rows - ehs / cond / intrablock carry K B, the latents are read from the staging buffer; the state, the LR
// anchor and the noise stay [B].  sampler_run_impl builds the StepPlan of the run piece by piece (run_check, run_operands, run_buffers,
// run_temb_table), then run_steps captures step_body(plan) - or reuses the graph when the plan is the stored one - and replays it.
struct RunArgs {
    mrisr_tensor* latents;
    const mrisr_tensor *lr, *noise, *ehs, *cond, *intrablock;
    int n_intrablock, K;
    bool pag;
};
// Step variants: what a step may leave out, decided per step on the host from the float32 rows of the run's tables (row i
// belongs to step i of the schedule, also under set_range); mrisr.step_variants states the same rule in Python.
//   STEP_REDUCED:  a guided / pag run with a schedule table whose row has g == 1 and s == 0 (pag alone: s == 0; phi does not matter): the forward
//                  runs on the conditional rows only - the last B T of the K B T - and the reduced step kernel steps from their prediction
//   STEP_NO_CNET:  a ControlNet and a conditioning table with c == 0: neither the ControlNet forward nor the residual adds are launched
//   STEP_NO_INTRA: adapter features and a conditioning table with a == 0: the UNet forward gets no features
// Without the option (or the table) every step is variant 0, the full step.
enum { STEP_REDUCED = 1, STEP_NO_CNET = 2, STEP_NO_INTRA = 4 };
static int step_variant(const mrisr_sampler* s, const StepPlan& p, int n_intra, int i) {
    int v = 0;
    if (p.d_sched && p.K > 1) {
        const float* r = s->sched.row(i);
        const bool pag_alone = p.pag && p.K == 2;
        if (r[1] == 0.f && (pag_alone || r[0] == 1.f)) v |= STEP_REDUCED;
    }
    if (p.d_cond) {
        const float* c = s->cond.row(i);
        if (p.cnet && c[0] == 0.f) v |= STEP_NO_CNET;
        if (n_intra > 0 && c[1] == 0.f) v |= STEP_NO_INTRA;
    }
    return v;
}
static long long numel(const mrisr_tensor* t) { long long k = 1; for (int i = 0; i < t->ndim; ++i) k *= t->shape[i]; return k; }
static mrisr_tensor plan_tensor(const PlanTensor& t, int cdt) {
    mrisr_tensor m{};
    m.data = const_cast<void*>(t.data); m.dtype = cdt; m.layout = MRISR_NHWC; m.ndim = 4;
    for (int i = 0; i < 4; ++i) m.shape[i] = t.shape[i];
    return m;
}

// argument checks; fills the plan's step configuration
static int run_check(mrisr_sampler* s, const RunArgs& a, StepPlan& p) {
    const int K = a.K;
    const bool guided = K > 1, pag = a.pag;
    const mrisr_tensor *latents = a.latents, *ehs = a.ehs, *cond = a.cond;
    MRISR_REQUIRE(s && latents && ehs, "null argument");
    MRISR_REQUIRE(latents->ndim == 4 && latents->dtype == MRISR_F32 && latents->layout == MRISR_NCHW, "latents: f32 NCHW");
    MRISR_REQUIRE(s->kind != MRISR_STEP_RESSHIFT || a.lr, "Res-SRDiff needs the LR anchor latents");
    MRISR_REQUIRE(!s->multistep() || !a.noise, "the multistep solvers are deterministic: step_noise is refused");
    MRISR_REQUIRE(!s->cnet || cond, "ControlNet needs the condition image");
    const bool cached = s->cache_interval > 1;
    if (pag) {
        MRISR_REQUIRE(K == 2 || K == 3, "pag run: the forward has 2B rows (pag alone) or 3B rows (with classifier-free guidance)");
        MRISR_REQUIRE(s->pag_mask != 0, "pag run: no applied block (mrisr_sampler_set_pag)");
    }
    const bool ctab = s->cond.on(), guess = ctab && s->cond_guess;
    Options o = current_options(s);
    o.pag_run = pag; o.cond_table = ctab; o.guess = guess;
    const char* conflict = option_conflict(*s->unet, o);
    MRISR_REQUIRE(!conflict, conflict);
    Model& U = *s->unet;
    if (ctab) {  // the table only supplies values: one this run cannot honour is refused
        MRISR_REQUIRE(s->cnet || !s->cond_c, "conditioning: rows with a controlnet scale (c) != 1 need a sampler with a ControlNet");
        MRISR_REQUIRE(s->cnet || !guess, "conditioning: guess mode needs a sampler with a ControlNet");
        MRISR_REQUIRE(a.n_intrablock > 0 || !s->cond_a, "conditioning: rows with an adapter scale (a) != 1 need a run with adapter features");
        MRISR_REQUIRE(!U.cond.on && (!s->cnet || !s->cnet->cond.on), "conditioning: a model handle already carries a conditioning state");
    }
    const bool guess_half = guess && K == 2 && !pag;  // the ControlNet runs on the B conditional rows only
    const bool sched = s->sched.on();
    if (sched) {  // the run kind comes from the entry point; the table only supplies the values, and a value this kind cannot honour is refused
        MRISR_REQUIRE(U.freeu.on || !s->sched_freeu, "schedule: FreeU columns other than 1 need FreeU on the UNet (mrisr_model_set_freeu)");
        MRISR_REQUIRE(pag || !s->sched_s, "schedule: rows with pag_scale (s) > 0 need a pag run (mrisr_sampler_run_pag)");
        MRISR_REQUIRE(K == 3 || (K == 2 && !pag) || !s->sched_g,
                      "schedule: rows with guidance_scale (g) != 1 need a run with an unconditional half (mrisr_sampler_run_guided, or "
                      "mrisr_sampler_run_pag with_cfg)");
    }
    const int B = (int)latents->shape[0], h = (int)latents->shape[2], w = (int)latents->shape[3];
    const int NB = K * B;  // rows of every forward (of the canvas; a tiled run multiplies them by T)
    const long long per = (long long)latents->shape[1] * h * w;
    const long long n = (long long)B * per;
    // every operand the step kernels index is checked against the latents here: the kernels themselves read
    // lr[i], noise[step * n + i] for i < n without bounds
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
        MRISR_REQUIRE(ehs->ndim == 3 && ehs->shape[0] == FB && ehs->shape[2] == U.cfg.cross_attention_dim,
                      "tiled run: encoder_hidden_states must be [NB*T, L, cross_attention_dim]: every forward row's context T times, sample-major");
        if (cond) MRISR_REQUIRE(cond->ndim == 4 && cond->shape[0] == FB && cond->shape[2] == 8 * fh && cond->shape[3] == 8 * fw,
                                "tiled run: controlnet_cond must be [NB*T, C, 8 t_h, 8 t_w]: the image cropped per tile");
        for (int i = 0; i < a.n_intrablock; ++i) {
            const mrisr_tensor& f = a.intrablock[i];
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
    if (a.lr) MRISR_REQUIRE(a.lr->dtype == MRISR_F32 && numel(a.lr) == n, "lr_latents: f32, same shape as latents");
    if (cond && guess_half)
        MRISR_REQUIRE(cond->ndim == 4 && cond->shape[0] == B && cond->shape[2] == 8 * h && cond->shape[3] == 8 * w,
                      "guided run in guess mode: controlnet_cond must be [B, C, 8h, 8w]: the ControlNet sees the conditional rows only");
    else if (cond && !tiled)
        MRISR_REQUIRE(cond->ndim == 4 && cond->shape[0] == NB && cond->shape[2] == 8 * h && cond->shape[3] == 8 * w,
                      pag ? "pag run: controlnet_cond must be [K B, C, 8h, 8w] (the [B] images K times)"
                      : guided ? "guided run: controlnet_cond must be [2B, C, 8h, 8w] (the [B] images twice)"
                             : "controlnet_cond must be [B, C, 8h, 8w] with the latents' batch");
    {
        int need = 0;  // slabs read: one per step, indexed by the step's position in the schedule, when its sigma != 0
        for (int i = s->first; i < s->last; ++i)
            if (s->sigma[i] != 0.f) need = i + 1;
        if (a.noise) {
            MRISR_REQUIRE(a.noise->dtype == MRISR_F32 && a.noise->ndim >= 1 && numel(a.noise) % n == 0,
                          "step_noise: f32, a stack of latents-shaped slabs");
            MRISR_REQUIRE(numel(a.noise) / n >= need, "step_noise has fewer slabs than the last stochastic step needs");
        }
    }
    for (int i = 0; i < a.n_intrablock && !tiled; ++i)
        MRISR_REQUIRE(a.intrablock[i].ndim == 4 && a.intrablock[i].shape[0] == NB,
                      pag ? "pag run: adapter features must be [K B, ...] (the [B] features K times)"
                      : guided ? "guided run: adapter features must be [2B, ...] (the [B] features twice)"
                             : "adapter features must carry the latents' batch");
    MRISR_REQUIRE(a.n_intrablock >= 0 && a.n_intrablock <= PLAN_MAX_INTRA, "more adapter features than a step plan holds");
    MRISR_REQUIRE(!s->cnet || s->cnet->num_skips() + 1 <= PLAN_MAX_RES, "more ControlNet residuals than a step plan holds");

    // a field that this configuration's launches do not take stays zero: changing it alone must not capture again
    p.kind = s->kind; p.K = K; p.pag = pag;
    p.B = B; p.T = T; p.C = Cl; p.h = h; p.w = w; p.fh = fh; p.fw = fw; p.L = (int)ehs->shape[1];
    p.cnet = s->cnet != nullptr;
    p.cdt = U.cfg.compute_dtype;
    p.first = s->first;
    p.x = static_cast<float*>(latents->data);
    p.lr = a.lr ? static_cast<const float*>(a.lr->data) : nullptr;
    p.noise = a.noise ? static_cast<const float*>(a.noise->data) : nullptr;
    p.d_coef = static_cast<const float*>(s->d_coef.p);
    p.d_step = static_cast<int*>(s->d_step.p);
    p.d_curt = static_cast<long long*>(s->d_curt.p);
    p.d_ts = static_cast<const long long*>(s->d_ts.p);
    if (s->kind == MRISR_STEP_DDPM) p.clip = s->clip;
    if (pag) p.pag_mask = s->pag_mask;
    if (sched && (guided || U.freeu.on)) {
        // a per-step schedule: the launches take the table's address, never its values - other values, same graph.  What chooses kernels
        // is here: the rescale kernel (some phi > 0) and FreeU's table mode (the UNet's workspace generation carries a marker for it)
        p.d_sched = static_cast<const float*>(s->sched.dev.p);
        p.sched_rows = s->n_steps;
        if (guided) p.sched_phi = s->sched_phi ? 1 : 0;
        if (U.freeu.on) p.freeu = 2;
    } else {
        if (guided) { p.guidance_scale = s->guidance_scale; p.guidance_rescale = s->guidance_rescale; }
        if (pag) p.pag_scale = s->pag_scale;
        if (U.freeu.on) {  // the four scalars the decoder's FreeU launches take by value (also in the UNet's workspace generation)
            p.freeu = 1;
            p.freeu_s[0] = U.freeu.s[0]; p.freeu_s[1] = U.freeu.s[1]; p.freeu_b[0] = U.freeu.b[0]; p.freeu_b[1] = U.freeu.b[1];
        }
    }
    if (ctab) {
        // the conditioning table: the launches take its address, never its values - other values, same graph.  What chooses launches is
        // here: table mode itself (the scaled adds; both workspace generations carry a marker for it), guess mode, the ControlNet's rows
        p.d_cond = static_cast<const float*>(s->cond.dev.p);
        p.cond_guess = guess ? 1 : 0;
        if (s->cnet) p.cnet_rows = guess_half ? B : FB;
    }
    if (s->cons.on()) {
        // the consistency launch runs on the canvas (tiles gather from it afterwards): its rules are checked against the canvas.  The launch takes
        // the table's address, never its values - other values, same graph; factor, filter and the two buffers' addresses choose the launch
        for (int i = 0; i < 4; ++i)
            MRISR_REQUIRE(latents->shape[i] == s->cons_shape[i], "consistency: the reference must have the shape of the latents");
        TRY(check_consistency_geometry(s->cons_factor, s->cons_filter, h, w));
        p.d_cons = static_cast<const float*>(s->cons.dev.p);
        p.cons_ref = s->cons_ref; p.cons_noise = s->cons_noise;
        p.cons_factor = s->cons_factor; p.cons_filter = s->cons_filter;
    }
    if (s->multistep()) {
        p.order = s->ms.order;
        p.final_zero = s->ms.final_zero; p.lower_order_final = s->ms.lower_order_final;
        p.n_disabled = (int)s->ms.disable_corrector.size();
        for (int i = 0; i < p.n_disabled && i < 32; ++i) p.disabled[i] = s->ms.disable_corrector[i];
    }
    if (cached) { p.cached = 1; p.cache_depth = s->cache_depth; }
    if (tiled) {
        p.tile_h = s->tile_h; p.tile_w = s->tile_w; p.tile_oh = s->tile_oh; p.tile_ow = s->tile_ow; p.tile_window = s->tile_window;
    }
    return 0;
}

// one-time (per run) timestep-invariant work: context projections, condition embedding, ControlNet residual buffers, feature conversion
static int run_operands(mrisr_sampler* s, const RunArgs& a, StepPlan& p, hipStream_t st) {
    Model& U = *s->unet;
    const int FB = p.K * p.B * p.T, esz = dtype_size(p.cdt);
    TRY(gemm_prepare());
    TRY(U.set_context(a.ehs, FB, p.fh, p.fw, st));
    if (s->cnet) {
        Model& C = *s->cnet;
        const int CB = p.cnet_rows ? p.cnet_rows : FB;  // guess mode under classifier-free guidance: the conditional rows, the last B
        mrisr_tensor ehs_c = *a.ehs;
        if (CB != FB) {
            ehs_c.shape[0] = CB;
            ehs_c.data = static_cast<char*>(a.ehs->data) + (size_t)(FB - CB) * a.ehs->shape[1] * a.ehs->shape[2] * dtype_size(a.ehs->dtype);
        }
        TRY(C.set_context(&ehs_c, CB, p.fh, p.fw, st));
        TRY(C.set_cond(a.cond, p.L, st));
        p.n_res = C.num_skips();
        s->res_bufs.resize(p.n_res + 1);
        for (int k = 0; k <= p.n_res; ++k) {  // the mid residual last
            int64_t shape[4];
            C.skip_shape(k, CB, p.fh, p.fw, shape);
            if (!s->res_bufs[k]) s->res_bufs[k].reset(new DevBuf());
            TRY(s->res_bufs[k]->reserve((size_t)shape[0] * shape[1] * shape[2] * shape[3] * esz, false));
            p.res[k].data = s->res_bufs[k]->p;
            for (int i = 0; i < 4; ++i) p.res[k].shape[i] = shape[i];
        }
    }
    p.n_intra = a.n_intrablock;
    s->intra_bufs.resize(a.n_intrablock);
    for (int i = 0; i < a.n_intrablock; ++i) {
        const mrisr_tensor& f = a.intrablock[i];
        MRISR_REQUIRE(f.ndim == 4, "adapter feature rank");
        p.intra[i].data = f.data;
        for (int k = 0; k < 4; ++k) p.intra[i].shape[k] = f.shape[k];
        if (f.layout == MRISR_NHWC && f.dtype == p.cdt) continue;
        if (!s->intra_bufs[i]) s->intra_bufs[i].reset(new DevBuf());
        TRY(s->intra_bufs[i]->reserve((size_t)f.shape[0] * f.shape[1] * f.shape[2] * f.shape[3] * esz, false));
        if (p.cdt == MRISR_F32) TRY(launch_nchw_to_nhwc<float>(f.data, f.dtype, s->intra_bufs[i]->p, (int)f.shape[0], (int)f.shape[1], (int)f.shape[2], (int)f.shape[3], st));
        else TRY(launch_nchw_to_nhwc<bf16>(f.data, f.dtype, s->intra_bufs[i]->p, (int)f.shape[0], (int)f.shape[1], (int)f.shape[2], (int)f.shape[3], st));
        p.intra[i].data = s->intra_bufs[i]->p;
    }
    // reduced steps forward a row window of the planned batch: its shapes are sized (bf16: tuned) here, before anything is captured
    bool any_reduced = false;
    for (int i = s->first; i < s->last; ++i) any_reduced |= (s->variant[i] & STEP_REDUCED) != 0;
    if (any_reduced) {
        TRY(U.check_window(p.B * p.T, st));
        if (s->cnet && !(p.cnet_rows && p.cnet_rows != FB)) TRY(s->cnet->check_window(p.B * p.T, st));
    }
    p.ws_gen_unet = U.ws_gen;
    p.ws_gen_cnet = s->cnet ? s->cnet->ws_gen : 0ull;
    return 0;
}

// the sampler's own buffers: the forward's output, tiles, feature cache, staging, multistep history, the step counter
static int run_buffers(mrisr_sampler* s, StepPlan& p, hipStream_t st) {
    Model& U = *s->unet;
    const int NB = p.K * p.B;
    const long long per = (long long)p.C * p.h * p.w, n = (long long)p.B * per;
    TRY(s->d_eps.reserve((size_t)NB * per * sizeof(float), false));
    p.d_eps = static_cast<float*>(s->d_eps.p);
    if (p.T > 1) {
        // the table is uploaded before any capture; the graph reads it from d_tiles at every replay.  s->tiles is pageable and rebuilt by the
        // next run: like the copy of ms_rows below, this relies on the runtime staging the copy before hipMemcpyAsync returns
        const size_t tile_elems = (size_t)NB * p.T * p.C * p.fh * p.fw;
        TRY(s->d_tiles.reserve(s->tiles.bytes(), false));
        TRY(s->d_xt.reserve(tile_elems * sizeof(float), false));
        TRY(s->d_et.reserve(tile_elems * sizeof(float), false));
        MRISR_CHECK_HIP(hipMemcpyAsync(s->d_tiles.p, s->tiles.words.data(), s->tiles.bytes(), hipMemcpyHostToDevice, st));
        const TileGrid g = s->tiles.grid(s->d_tiles.p);
        p.tile_oy = g.oy; p.tile_ox = g.ox; p.tile_nwy = g.nwy; p.tile_nwx = g.nwx;
        p.tile_ky = g.ky; p.tile_kx = g.kx; p.tile_vec4 = g.vec4;
        p.d_xt = static_cast<float*>(s->d_xt.p); p.d_et = static_cast<float*>(s->d_et.p);
    }
    if (p.cached) {  // reserved here, before any capture; written by the first step of every run before anything reads it
        int64_t cs[4];
        TRY(U.cache_shape(p.cache_depth, NB, p.h, p.w, cs));
        TRY(s->d_cache.reserve((size_t)cs[0] * cs[1] * cs[2] * cs[3] * dtype_size(p.cdt), false));
        p.d_cache = s->d_cache.p;
    }
    if (p.K > 1) {
        // [x; x] ([x; x; x]) once per run; from then on the fused step itself writes every new state to every part
        TRY(s->d_x2.reserve((size_t)p.K * n * sizeof(float), false));
        for (int k = 0; k < p.K; ++k)
            MRISR_CHECK_HIP(hipMemcpyAsync(static_cast<float*>(s->d_x2.p) + (size_t)k * n, p.x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
        p.d_x2 = static_cast<float*>(s->d_x2.p);
    }
    if (s->multistep()) {
        // this range's rows, and a zeroed history: the rows of a cold start carry zero coefficients for the absent terms, and
        // 0 x (whatever an earlier run or the allocator left) is not 0
        TRY(s->d_hist.reserve((size_t)p.order * n * sizeof(float), false));
        MRISR_CHECK_HIP(hipMemsetAsync(s->d_hist.p, 0, (size_t)p.order * n * sizeof(float), st));
        p.hist = static_cast<float*>(s->d_hist.p);
        if (s->kind == MRISR_STEP_UNIPC) {
            TRY(s->d_xc.reserve((size_t)n * sizeof(float), false));
            MRISR_CHECK_HIP(hipMemsetAsync(s->d_xc.p, 0, (size_t)n * sizeof(float), st));
            p.xc = static_cast<float*>(s->d_xc.p);
        }
        // ms_rows is pageable and may be rebuilt (set_solver / set_range) right after this call returns: staged like the tables' rows
        // (StepTable::upload) and the copy of s->first below
        MRISR_CHECK_HIP(hipMemcpyAsync(s->d_coef.p, s->ms_rows.data(), sizeof(float) * s->ms_rows.size(), hipMemcpyHostToDevice, st));
    }
    if (p.d_sched) TRY(s->sched.upload(s->n_steps, st));
    if (p.d_cond) TRY(s->cond.upload(s->n_steps, st));
    if (p.d_cons) TRY(s->cons.upload(s->n_steps, st));
    MRISR_CHECK_HIP(hipMemsetAsync(s->d_step.p, 0, 16, st));
    MRISR_CHECK_HIP(hipMemcpyAsync(s->d_step.p, &s->first, sizeof(int), hipMemcpyHostToDevice, st));
    return 0;
}

// the time embedding of every step of this run, once (it depends on the timestep only): sinusoid -> MLP -> the 22 per-resnet projections for
// all rows at once instead of three GEMVs over 50 MB of weights in every step.  MRISR_TEMB_TABLE=0 / mrisr_debug_temb_table(0): per step.
// Leaves the models pointing at the tables: the caller's guard clears that when the run returns.
static int run_temb_table(mrisr_sampler* s, StepPlan& p, hipStream_t st) {
    if (!temb_table_enabled()) return 0;
    const int rows = s->last - s->first;
    auto build = [&](Model& M, DevBuf& buf) -> int {
        const size_t scratch = (size_t)64 * M.cfg.block_out_channels[0] * 9;
        TRY(buf.reserve((scratch + (size_t)rows * M.tproj_total) * sizeof(float), false));
        float* sc = static_cast<float*>(buf.p);
        TRY(M.build_tproj_table(static_cast<const long long*>(s->d_ts.p) + s->first, rows, sc, sc + scratch, st));
        M.tproj_table = sc + scratch; M.tproj_step = static_cast<const int*>(s->d_step.p); M.tproj_first = s->first;
        return 0;
    };
    TRY(build(*s->unet, s->tp_unet));
    p.tproj_unet = s->unet->tproj_table;
    if (s->cnet) { TRY(build(*s->cnet, s->tp_cnet)); p.tproj_cnet = s->cnet->tproj_table; }
    return 0;
}

// ONE step: everything here comes from the plan (C: the ControlNet when p.cnet).  Workspaces are planned (set_context in run_operands), so
// a captured body performs launches only.
// variant: the STEP_* bits of this step.  A reduced step runs everything on the row window [FB - B T, FB) of the planned batch: the last part of
// the staging buffer, of the tile batch and of d_eps.
static int step_body(const StepPlan& p, Model& U, Model* C, int cache_mode, int variant, hipStream_t st) {
    const int NB = p.K * p.B, FB = NB * p.T;
    const long long per = (long long)p.C * p.h * p.w, n = (long long)p.B * per;
    const bool tiled = p.T > 1;
    const bool reduced = (variant & STEP_REDUCED) != 0, with_cnet = p.cnet && !(variant & STEP_NO_CNET);
    const int n_intra = (variant & STEP_NO_INTRA) ? 0 : p.n_intra;
    MRISR_REQUIRE(!reduced || (p.K > 1 && cache_mode == CACHE_NONE), "reduced step: a guided or pag run without a feature cache");
    const int WB = reduced ? p.B * p.T : FB;   // rows of this step's forwards
    const RowWindow win{FB - WB, FB};
    const size_t win_off = (size_t)win.lo * p.C * p.fh * p.fw;  // the window's first element in a [FB, C, fh, fw] buffer
    const size_t part_off = reduced ? (size_t)(p.K - 1) * n : 0;  // ... and in a [K B, C, h, w] canvas buffer (the same number when not tiled)
    mrisr_tensor tt{};
    tt.data = p.d_curt; tt.dtype = MRISR_I64; tt.ndim = 0;
    const float* canvas = p.K > 1 ? p.d_x2 : p.x;  // [NB, C, h, w]: what the forwards read, or what a tiled step gathers from
    mrisr_tensor xin{};                            // what the forwards read
    xin.data = (tiled ? p.d_xt : const_cast<float*>(canvas)) + win_off;
    xin.dtype = MRISR_F32; xin.layout = MRISR_NCHW; xin.ndim = 4;
    xin.shape[0] = WB; xin.shape[1] = p.C; xin.shape[2] = p.fh; xin.shape[3] = p.fw;
    mrisr_tensor eps_t = xin;
    eps_t.data = (tiled ? p.d_et : p.d_eps) + win_off;
    TileGrid tg;
    if (tiled) {
        tg.H = p.h; tg.W = p.w; tg.th = p.fh; tg.tw = p.fw; tg.ky = p.tile_ky; tg.kx = p.tile_kx;
        tg.oy = p.tile_oy; tg.ox = p.tile_ox; tg.nwy = p.tile_nwy; tg.nwx = p.tile_nwx;
        tg.vec4 = p.tile_vec4 != 0;
    }
    mrisr_tensor res[PLAN_MAX_RES], intra[PLAN_MAX_INTRA];
    for (int k = 0; k <= p.n_res && p.cnet; ++k) {
        res[k] = plan_tensor(p.res[k], p.cdt);
        if (reduced) res[k].shape[0] = WB;  // the residuals of the window's rows, at the head of each buffer
    }
    for (int i = 0; i < n_intra; ++i) {
        intra[i] = plan_tensor(p.intra[i], p.cdt);
        if (reduced) {  // the features of the window's rows
            const PlanTensor& f = p.intra[i];
            intra[i].shape[0] = WB;
            intra[i].data = static_cast<char*>(intra[i].data) + (size_t)win.lo * f.shape[1] * f.shape[2] * f.shape[3] * dtype_size(p.cdt);
        }
    }
    UNetCache fc;
    fc.mode = cache_mode; fc.depth = p.cache_depth; fc.p = p.d_cache;

    hipLaunchKernelGGL(load_t_kernel, dim3(1), dim3(1), 0, st, p.d_curt, p.d_ts, static_cast<const int*>(p.d_step));
    // (a reduced tiled step gathers from the last part of the staging buffer only, and blends into the window of d_eps)
    if (tiled) TRY(launch_tile_gather(canvas + part_off, p.d_xt + win_off, tg, reduced ? p.B : NB, p.C, st));
    if (with_cnet) {
        mrisr_tensor cin = xin;
        const bool cond_rows = p.cnet_rows && p.cnet_rows != FB;  // guess mode under classifier-free guidance: the ControlNet is planned for, and
        if (cond_rows) {                                          // runs on, the last B rows of the staging buffer - a reduced step's window
            cin.shape[0] = p.cnet_rows;
            cin.data = const_cast<float*>(canvas) + (size_t)(FB - p.cnet_rows) * per;
        }
        TRY(C->forward_controlnet(&cin, &tt, nullptr, nullptr, 1.0f, res, p.n_res, &res[p.n_res], st, reduced && !cond_rows ? &win : nullptr));
    }
    TRY(U.forward_unet(&xin, &tt, nullptr, with_cnet ? res : nullptr, with_cnet ? p.n_res : 0, with_cnet ? &res[p.n_res] : nullptr, intra, n_intra,
                       &eps_t, st, p.cached ? &fc : nullptr, reduced ? &win : nullptr));
    if (tiled) TRY(launch_tile_blend(p.d_et + win_off, p.d_eps + part_off, tg, reduced ? p.B : NB, p.C, st));
    StepArgs a;
    a.kind = p.kind; a.K = p.K;
    a.x = p.x; a.xK = p.d_x2; a.eps = p.d_eps + part_off;
    a.lr = p.lr; a.noise = p.noise; a.coef = p.d_coef; a.step = p.d_step; a.clip = p.clip;
    a.B = p.B; a.per = per;
    a.ms = MsBuf{p.hist, p.xc, p.order};
    if (p.K > 1 && !reduced) {
        // K = 3: [eps_p; eps_u; eps_c].  K = 2 of a pag run: [eps_p; eps_c], the guided step with eps_u := eps_p and g := 1 + s
        // with a schedule table the kernel reads the three scalars from row *d_step (and forms 1 + s itself): the plan holds zeros for them
        a.pag_alone = p.pag && p.K == 2 ? 1 : 0;
        a.g = a.pag_alone ? 1.f + p.pag_scale : p.guidance_scale;
        a.s = p.K == 3 ? p.pag_scale : 0.f;
        a.phi = p.guidance_rescale;
        a.sched = p.d_sched; a.sched_phi = p.sched_phi;
    }
    TRY(launch_step(a, reduced, st));
    if (p.d_cons) {
        // low-frequency consistency: on the new state, row *d_step - so before the counter advances.  Every part of the
        // staging buffer receives the result, also on a reduced step
        ConsistArgs c;
        c.x = p.x; c.xK = p.d_x2; c.K = p.K; c.ref = p.cons_ref; c.lr = p.lr; c.noise = p.cons_noise;
        c.table = p.d_cons; c.step = p.d_step;
        c.B = p.B; c.C = p.C; c.h = p.h; c.w = p.w; c.factor = p.cons_factor; c.filter = p.cons_filter;
        TRY(launch_consistency(c, st));
    }
    return launch_advance_step(p.d_step, st);
}

// capture and replay: the stored graphs serve this run exactly when they were captured from an equal plan.  One graph per step variant (and,
// with a feature cache, the shallow step), each captured the first time a run needs it - all of them before the run's first launch - from the
// same plan; which one a step replays is decided here, on the host.
static int run_steps(mrisr_sampler* s, const StepPlan& p, int use_graph, hipStream_t st) {
    Model& U = *s->unet;
    const bool cached = p.cached != 0;
    auto mode_of = [&](int i) { return !cached ? CACHE_NONE : ((i - s->first) % s->cache_interval == 0 ? CACHE_STORE : CACHE_USE); };
    const int FB = p.K * p.B * p.T;
    unsigned used = 0;
    for (int k = 0; k < 4; ++k) s->stats[k] = 0;
    for (int i = s->first; i < s->last; ++i) {
        const int v = s->variant[i];
        used |= 1u << v;
        s->stats[0] += (v & STEP_REDUCED) ? p.B * p.T : FB;
        s->stats[1] += p.cnet && !(v & STEP_NO_CNET) ? 1 : 0;
        s->stats[2] += p.n_intra > 0 && !(v & STEP_NO_INTRA) ? 1 : 0;
    }
    for (int v = 0; v < 8; ++v) s->stats[3] += (used >> v) & 1u;
    if (!use_graph) {
        for (int i = s->first; i < s->last; ++i) TRY(step_body(p, U, s->cnet, mode_of(i), s->variant[i], st));
        return 0;
    }
    if (!same_plan(s->plan, p)) {
        s->drop_graphs();
        s->plan = p;  // (now, not after the captures: a graph that exists was captured from s->plan, also when a capture below fails)
    }
    auto capture = [&](int cache_mode, int variant, hipGraphExec_t* exec) -> int {
        hipGraph_t graph = nullptr;
        MRISR_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        int rc = step_body(p, U, s->cnet, cache_mode, variant, st);
        hipError_t e = hipStreamEndCapture(st, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        MRISR_CHECK_HIP(e);
        MRISR_CHECK_HIP(hipGraphInstantiate(exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        ++s->n_captures;
        return 0;
    };
    if (cached) {  // both steps of a cached run, whatever its length: a change of range replays them
        if (!s->exec[0] || !s->exec_shallow) {
            s->drop_graphs();
            TRY(capture(CACHE_STORE, 0, &s->exec[0]));
            TRY(capture(CACHE_USE, 0, &s->exec_shallow));
        }
    } else {
        if (s->first == s->last && !s->exec[0]) TRY(capture(CACHE_NONE, 0, &s->exec[0]));  // (an empty range captures the full step, as ever)
        for (int i = s->first; i < s->last; ++i)  // in the order of first use
            if (!s->exec[s->variant[i]]) TRY(capture(CACHE_NONE, s->variant[i], &s->exec[s->variant[i]]));
    }
    for (int i = s->first; i < s->last; ++i)
        MRISR_CHECK_HIP(hipGraphLaunch(mode_of(i) == CACHE_USE ? s->exec_shallow : s->exec[s->variant[i]], st));
    return 0;
}

static int sampler_run_impl(mrisr_sampler* s, const RunArgs& a, int use_graph, void* stream) {
    API_BEGIN
    StepPlan p = new_step_plan();
    TRY(run_check(s, a, p));
    s->variant.assign(s->n_steps, 0);
    for (int i = s->first; i < s->last && s->skip; ++i) s->variant[i] = (unsigned char)step_variant(s, p, a.n_intrablock, i);
    hipStream_t user = (hipStream_t)stream;
    hipStream_t st = user;
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
    Model& U = *s->unet;
    // What this run parks on the model handles, cleared - exactly what was set - when this call returns, also on an error path: plain
    // forwards on the handles stay as they were.  All of it is set before the workspaces are planned (the plans and their keys see it).
    struct RunGuard {
        Model& U;
        Model* C;
        bool pag = false, freeu = false, cond = false, tproj = false;
        ~RunGuard() {
            if (pag) U.pag = PagState();
            if (freeu) { U.freeu.sched = nullptr; U.freeu.step = nullptr; }
            if (cond) { U.cond = CondState(); if (C) C->cond = CondState(); }
            if (tproj) { U.tproj_table = nullptr; if (C) C->tproj_table = nullptr; }
        }
    } guard{U, s->cnet};
    if (a.pag) {  // perturbed rows first: samples [0, B) of the forward, [0, B T) of a tiled one
        MRISR_REQUIRE(!U.pag.on(), "pag run: the UNet handle already carries a pag state (mrisr_model_set_pag); clear it first");
        guard.pag = true;
        U.pag.mask = s->pag_mask; U.pag.first = 0; U.pag.count = p.B * p.T;
    }
    if (p.freeu == 2) {  // FreeU from the schedule table: the UNet's launches read row *d_step instead of their four values
        guard.freeu = true;
        U.freeu.sched = p.d_sched; U.freeu.step = static_cast<const int*>(s->d_step.p);
    }
    if (p.d_cond) {
        // the conditioning table: the UNet adds residuals and features with the scaled multi-tensor add and the ControlNet writes its
        // outputs where that add reads them
        guard.cond = true;
        CondState cs;
        cs.on = true; cs.guess = p.cond_guess != 0;
        cs.table = p.d_cond; cs.step = static_cast<const int*>(s->d_step.p);
        const int n_down = s->cnet ? s->cnet->num_skips() : 0;
        for (int k = 0; k <= n_down; ++k) cs.w[k] = 1.f;
        if (cs.guess) guess_mode_weights(n_down, cs.w);
        if (s->cnet) { s->cnet->cond = cs; s->cnet->cond.row_lo = s->cnet->cond.row_hi = 0; }
        if (p.cnet_rows && p.cnet_rows != p.K * p.B * p.T) { cs.row_lo = p.K * p.B * p.T - p.cnet_rows; cs.row_hi = p.K * p.B * p.T; }
        U.cond = cs;
    }
    TRY(run_operands(s, a, p, st));
    TRY(run_buffers(s, p, st));
    guard.tproj = true;  // the models must not keep pointing at this sampler's table after the run (plain forward calls compute their own)
    TRY(run_temb_table(s, p, st));
    TRY(run_steps(s, p, use_graph, st));
    if (st != user) {
        MRISR_CHECK_HIP(hipEventRecord(s->ev_out, st));
        MRISR_CHECK_HIP(hipStreamWaitEvent(user, s->ev_out, 0));
    }
    return 0;
    API_END
}

// ---- the single-step test entries (mrisr_op_*_step): each fills an OpStep, op_step runs it.  K = 1: the plain multistep step; K = 2 / 3: the
// guided / three-way step on caller buffers xK / eps [K B].
struct OpStep {
    const char* who = "";         // the message prefix of the entry
    int K = 1, kind = 0;
    mrisr_tensor* x = nullptr;
    mrisr_tensor* xK = nullptr;
    const mrisr_tensor* eps = nullptr;
    const mrisr_tensor* lr = nullptr;
    const mrisr_tensor* noise = nullptr;
    const float* row_host = nullptr;  // `width` floats, this step kind's row: placed at row `slot` of a zeroed table
    int width = 0, slot = 0;          // the kernel sees the step counter `slot`
    mrisr_tensor* hist = nullptr;     // the multistep kinds' ring and corrected state
    mrisr_tensor* xc = nullptr;
    int order = 0;
    float clip = 0.f, g = 0.f, s = 0.f, phi = 0.f;
    const float* sched_host = nullptr;  // K > 1: a schedule table of n_rows rows, uploaded; the kernel reads {g, s, phi} from its row `slot`
    int n_rows = 0, pag_alone = 0;      // and g / s / phi are not read
    bool reduced = false;               // K > 1: the reduced step - eps is the conditional prediction alone, [B]
    void* stream = nullptr;
};
static int op_step(const OpStep& o) {
    const int K = o.K, slot = o.slot;
    const std::string w = std::string(o.who) + ": ", sK = std::to_string(K);
    const std::string eps_name = K == 3 ? "eps3" : (K == 2 ? "eps2" : "eps");
    const bool multistep = o.hist != nullptr;
    MRISR_REQUIRE(o.x->ndim == 4 && o.x->dtype == MRISR_F32 && o.x->shape[0] > 0, w + "x must be f32 [B, C, h, w]");
    const int B = (int)o.x->shape[0];
    const long long n = numel(o.x), per = n / B;
    if (multistep) MRISR_REQUIRE(per % 4 == 0, w + "C*h*w must be a multiple of 4");
    if (o.reduced) MRISR_REQUIRE(o.eps->dtype == MRISR_F32 && numel(o.eps) == n, w + "eps must be f32 [B, C, h, w]: the conditional prediction");
    else MRISR_REQUIRE(o.eps->dtype == MRISR_F32 && numel(o.eps) == K * n, w + eps_name + " must be f32 [" + (K > 1 ? sK : "") + "B, C, h, w]");
    if (o.xK) MRISR_REQUIRE(o.xK->dtype == MRISR_F32 && numel(o.xK) == K * n, w + "the staging buffer must be f32 [" + sK + "B, C, h, w]");
    if (o.lr) MRISR_REQUIRE(o.lr->dtype == MRISR_F32 && numel(o.lr) == n, w + "lr must be f32 [B, C, h, w]");
    // (the kernel reads slab `slot` of the noise: the single-slab entries run at slot 0, the scheduled one hands in slot + 1 slabs)
    if (o.noise) MRISR_REQUIRE(o.noise->dtype == MRISR_F32 && numel(o.noise) == (long long)(slot + 1) * n,
                               w + (slot ? "noise must be f32 [slot + 1, B, C, h, w]: one slab per step up to this one" : "noise must be one f32 [B, C, h, w] slab"));
    if (multistep) MRISR_REQUIRE(o.hist->dtype == MRISR_F32 && numel(o.hist) == (long long)o.order * n, w + "hist must be f32 [order, B, C, h, w]");
    if (o.xc) MRISR_REQUIRE(o.xc->dtype == MRISR_F32 && numel(o.xc) == n, w + "xc must be f32 [B, C, h, w]");
    hipStream_t st = (hipStream_t)o.stream;
    // the table's row pitch of this kind (load_step_row / multistep_value4): at slot 0, where the first-order entries run, any pitch serves
    const int pitch = multistep ? MS_ROW : (o.kind == MRISR_STEP_DDIM ? 2 : (o.kind == MRISR_STEP_RESSHIFT ? 4 : 8));
    std::vector<float> rows((size_t)(slot + 1) * pitch, 0.f);
    std::copy(o.row_host, o.row_host + o.width, rows.begin() + (size_t)slot * pitch);
    DevBuf d_rows, d_step, d_sched;
    TRY(d_rows.reserve(sizeof(float) * rows.size(), false));
    TRY(d_step.reserve(16, true));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_rows.p, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemsetAsync(d_step.p, 0, 16, st));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_step.p, &slot, sizeof(int), hipMemcpyHostToDevice, st));
    auto f32 = [](const mrisr_tensor* t) { return t ? static_cast<float*>(t->data) : nullptr; };
    StepArgs a;
    a.kind = o.kind; a.K = K;
    a.x = f32(o.x); a.xK = f32(o.xK); a.eps = f32(o.eps); a.lr = f32(o.lr); a.noise = f32(o.noise);
    a.coef = static_cast<const float*>(d_rows.p); a.step = static_cast<const int*>(d_step.p);
    a.clip = o.clip; a.g = o.g; a.s = o.s; a.phi = o.phi;
    a.B = B; a.per = per;
    a.ms = MsBuf{f32(o.hist), f32(o.xc), o.order};
    if (o.sched_host) {
        TRY(d_sched.reserve(sizeof(float) * 8 * (size_t)o.n_rows, false));
        MRISR_CHECK_HIP(hipMemcpyAsync(d_sched.p, o.sched_host, sizeof(float) * 8 * (size_t)o.n_rows, hipMemcpyHostToDevice, st));
        a.sched = static_cast<const float*>(d_sched.p);
        a.pag_alone = o.pag_alone;
        for (int i = 0; i < o.n_rows; ++i) a.sched_phi |= o.sched_host[8 * (size_t)i + 2] > 0.f ? 1 : 0;
    }
    TRY(launch_step(a, o.reduced, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}
static int row_width(int step_kind) { return step_kind == MRISR_STEP_DDIM ? 2 : (step_kind == MRISR_STEP_RESSHIFT ? 4 : 5); }

extern "C" {

int mrisr_sampler_run(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                      const mrisr_tensor* step_noise, const mrisr_tensor* ehs, const mrisr_tensor* cond,
                      const mrisr_tensor* intrablock, int n_intrablock, int use_graph, void* stream) {
    return sampler_run_impl(s, RunArgs{latents, lr_latents, step_noise, ehs, cond, intrablock, n_intrablock, 1, false}, use_graph, stream);
}
int mrisr_sampler_run_guided(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents,
                             const mrisr_tensor* step_noise, const mrisr_tensor* ehs2, const mrisr_tensor* cond2,
                             const mrisr_tensor* intrablock2, int n_intrablock, int use_graph, void* stream) {
    return sampler_run_impl(s, RunArgs{latents, lr_latents, step_noise, ehs2, cond2, intrablock2, n_intrablock, 2, false}, use_graph, stream);
}
int mrisr_sampler_run_pag(mrisr_sampler* s, mrisr_tensor* latents, const mrisr_tensor* lr_latents, const mrisr_tensor* step_noise,
                          const mrisr_tensor* ehsK, const mrisr_tensor* condK, const mrisr_tensor* intrablockK, int n_intrablock, int with_cfg,
                          int use_graph, void* stream) {
    return sampler_run_impl(s, RunArgs{latents, lr_latents, step_noise, ehsK, condK, intrablockK, n_intrablock, with_cfg ? 3 : 2, true}, use_graph,
                            stream);
}

// the guided step alone, on caller buffers (parity test): coef_row_host is this step kind's coefficient row (2 / 4 / 5 floats)
int mrisr_op_guided_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x2, const mrisr_tensor* eps2, const mrisr_tensor* lr,
                         const mrisr_tensor* noise, const float* coef_row_host, float clip, float guidance_scale,
                         float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && x2 && eps2 && coef_row_host, "guided step: null argument");
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DDPM, "guided step: unknown step kind");
    OpStep o;
    o.who = "guided step"; o.K = 2; o.kind = step_kind; o.stream = stream;
    o.x = x; o.xK = x2; o.eps = eps2; o.lr = lr; o.noise = noise;
    o.row_host = coef_row_host; o.width = row_width(step_kind);
    o.clip = clip; o.g = guidance_scale; o.phi = guidance_rescale;
    return op_step(o);
    API_END
}
// the three-way step alone: as mrisr_op_guided_step with x3 / eps3 [3B] = [perturbed; uncond; cond]
int mrisr_op_pag_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x3, const mrisr_tensor* eps3, const mrisr_tensor* lr,
                      const mrisr_tensor* noise, const float* coef_row_host, float clip, float guidance_scale, float pag_scale,
                      float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && x3 && eps3 && coef_row_host, "pag step: null argument");
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DDPM, "pag step: unknown step kind");
    OpStep o;
    o.who = "pag step"; o.K = 3; o.kind = step_kind; o.stream = stream;
    o.x = x; o.xK = x3; o.eps = eps3; o.lr = lr; o.noise = noise;
    o.row_host = coef_row_host; o.width = row_width(step_kind);
    o.clip = clip; o.g = guidance_scale; o.s = pag_scale; o.phi = guidance_rescale;
    return op_step(o);
    API_END
}
// the multistep step alone (parity test): row_host = one 16-float row; slot = the step counter the kernel sees; x2 given: the guided form
int mrisr_op_multistep_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x2, const mrisr_tensor* eps, const mrisr_tensor* lr,
                            mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot, float guidance_scale,
                            float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && eps && hist && row_host, "multistep step: null argument");
    MRISR_REQUIRE(step_kind == MRISR_STEP_UNIPC || step_kind == MRISR_STEP_DPMSOLVERPP, "multistep step: UniPC or DPM-Solver++");
    MRISR_REQUIRE(solver_order >= 1 && solver_order <= 3 && slot >= 0 && slot < 1024, "multistep step: solver order 1..3, slot 0..1023");
    MRISR_REQUIRE((step_kind == MRISR_STEP_UNIPC) == (xc != nullptr), "multistep step: the corrected-state buffer belongs to UniPC");
    OpStep o;
    o.who = "multistep step"; o.K = x2 ? 2 : 1; o.kind = step_kind; o.stream = stream;
    o.x = x; o.xK = x2; o.eps = eps; o.lr = lr;
    o.row_host = row_host; o.width = MS_ROW; o.slot = slot;
    o.hist = hist; o.xc = xc; o.order = solver_order;
    o.g = guidance_scale; o.phi = guidance_rescale;
    return op_step(o);
    API_END
}
// the three-way step of the multistep kinds alone: mrisr_op_multistep_step's guided form with x3 / eps3 [3B]
int mrisr_op_pag_multistep_step(int step_kind, mrisr_tensor* x, mrisr_tensor* x3, const mrisr_tensor* eps3, const mrisr_tensor* lr,
                                mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot, float guidance_scale,
                                float pag_scale, float guidance_rescale, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && x3 && eps3 && hist && row_host, "pag multistep step: null argument");
    MRISR_REQUIRE(step_kind == MRISR_STEP_UNIPC || step_kind == MRISR_STEP_DPMSOLVERPP, "pag multistep step: UniPC or DPM-Solver++");
    MRISR_REQUIRE(solver_order >= 1 && solver_order <= 3 && slot >= 0 && slot < 1024, "pag multistep step: solver order 1..3, slot 0..1023");
    MRISR_REQUIRE((step_kind == MRISR_STEP_UNIPC) == (xc != nullptr), "pag multistep step: the corrected-state buffer belongs to UniPC");
    OpStep o;
    o.who = "pag multistep step"; o.K = 3; o.kind = step_kind; o.stream = stream;
    o.x = x; o.xK = x3; o.eps = eps3; o.lr = lr;
    o.row_host = row_host; o.width = MS_ROW; o.slot = slot;
    o.hist = hist; o.xc = xc; o.order = solver_order;
    o.g = guidance_scale; o.s = pag_scale; o.phi = guidance_rescale;
    return op_step(o);
    API_END
}
// the guided step with its three scalars read from a schedule table (parity test): the K = 2 step of classifier-free guidance, the K = 2
// step of pag alone (pag_alone: g = 1 + s of the row) or the K = 3 step, of any step kind, on caller buffers at step counter `slot`.
// row_host: this kind's coefficient row (2 / 4 / 5 floats; 16 for the multistep kinds, which also take hist, UniPC xc, and solver_order).
// sched_host: n_rows rows of 8 floats; the rescale kernel runs iff some row has phi > 0, as in a run
int mrisr_op_scheduled_step(int step_kind, int K, int pag_alone, mrisr_tensor* x, mrisr_tensor* xK, const mrisr_tensor* epsK, const mrisr_tensor* lr,
                            const mrisr_tensor* noise, mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot,
                            float clip, const float* sched_host, int n_rows, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && xK && epsK && row_host && sched_host, "scheduled step: null argument");
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DPMSOLVERPP, "scheduled step: unknown step kind");
    MRISR_REQUIRE(K == 2 || K == 3, "scheduled step: 2 or 3 parts");
    MRISR_REQUIRE(!pag_alone || K == 2, "scheduled step: pag alone is the step on 2 parts");
    MRISR_REQUIRE(n_rows >= 1 && n_rows <= 1024 && slot >= 0 && slot < n_rows, "scheduled step: 1..1024 rows, slot inside the table");
    TRY(check_schedule_rows(sched_host, n_rows));
    const bool multistep = step_kind > MRISR_STEP_DDPM;
    if (multistep) {
        MRISR_REQUIRE(hist && !noise, "scheduled step: the multistep kinds take the history ring and no noise");
        MRISR_REQUIRE(solver_order >= 1 && solver_order <= 3, "scheduled step: solver order 1..3");
        MRISR_REQUIRE((step_kind == MRISR_STEP_UNIPC) == (xc != nullptr), "scheduled step: the corrected-state buffer belongs to UniPC");
    } else
        MRISR_REQUIRE(!hist && !xc, "scheduled step: hist / xc belong to the multistep kinds");
    OpStep o;
    o.who = "scheduled step"; o.K = K; o.kind = step_kind; o.stream = stream;
    o.x = x; o.xK = xK; o.eps = epsK; o.lr = lr; o.noise = noise;
    o.row_host = row_host; o.width = multistep ? MS_ROW : row_width(step_kind); o.slot = slot;
    o.hist = hist; o.xc = xc; o.order = multistep ? solver_order : 0;
    o.clip = clip;
    o.sched_host = sched_host; o.n_rows = n_rows; o.pag_alone = pag_alone ? 1 : 0;
    return op_step(o);
    API_END
}

// the reduced step alone (parity test): the step of any kind from the conditional prediction eps [B] on caller buffers at
// step counter `slot`, the new x to x and to all K parts of xK [K B].  row_host, hist, xc, solver_order, noise: as mrisr_op_scheduled_step
int mrisr_op_reduced_step(int step_kind, int K, mrisr_tensor* x, mrisr_tensor* xK, const mrisr_tensor* eps, const mrisr_tensor* lr,
                          const mrisr_tensor* noise, mrisr_tensor* hist, mrisr_tensor* xc, const float* row_host, int solver_order, int slot,
                          float clip, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && xK && eps && row_host, "reduced step: null argument");
    MRISR_REQUIRE(step_kind >= MRISR_STEP_DDIM && step_kind <= MRISR_STEP_DPMSOLVERPP, "reduced step: unknown step kind");
    MRISR_REQUIRE(K == 2 || K == 3, "reduced step: 2 or 3 parts");
    MRISR_REQUIRE(slot >= 0 && slot < 1024, "reduced step: slot 0..1023");
    const bool multistep = step_kind > MRISR_STEP_DDPM;
    if (multistep) {
        MRISR_REQUIRE(hist && !noise, "reduced step: the multistep kinds take the history ring and no noise");
        MRISR_REQUIRE(solver_order >= 1 && solver_order <= 3, "reduced step: solver order 1..3");
        MRISR_REQUIRE((step_kind == MRISR_STEP_UNIPC) == (xc != nullptr), "reduced step: the corrected-state buffer belongs to UniPC");
    } else
        MRISR_REQUIRE(!hist && !xc, "reduced step: hist / xc belong to the multistep kinds");
    OpStep o;
    o.who = "reduced step"; o.K = K; o.kind = step_kind; o.stream = stream; o.reduced = true;
    o.x = x; o.xK = xK; o.eps = eps; o.lr = lr; o.noise = noise;
    o.row_host = row_host; o.width = multistep ? MS_ROW : row_width(step_kind); o.slot = slot;
    o.hist = hist; o.xc = xc; o.order = multistep ? solver_order : 0;
    o.clip = clip;
    return op_step(o);
    API_END
}
}  // extern "C"
