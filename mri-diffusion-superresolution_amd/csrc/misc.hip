// Small / bandwidth-bound kernels: time-embedding GEMV, direct convolutions for tiny channel counts,
// NCHW<->NHWC boundary conversion, weight packers.  (The fused sampler steps live in sampler.hip.)
#include "common.h"
#include "prof.h"

namespace mrisr {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------
// y[b][n] = sum_k act(x[b][k]) W[n][k] + bias[n];  one wave per output column n, RB rows at a time.
// Weight-streaming (each W row read once, 16 B per lane); x is tiny and L1/L2 resident.
// ------------------------------------------------------------------------------------------------
template <typename T, int RB>
__global__ __launch_bounds__(256) void gemv_rows_kernel(const float* __restrict__ x, int ldx,
                                                        const T* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int ldy, int rows, int N, int K,
                                                        int silu_in) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    for (int r0 = 0; r0 < rows; r0 += RB) {
        float acc[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) acc[r] = 0.f;
        for (int k = lane * VE; k < K; k += 64 * VE) {
            float wv[VE];
            if constexpr (sizeof(T) == 2) {
                const bf16x8 t = *reinterpret_cast<const bf16x8*>(w + (size_t)n * K + k);
#pragma unroll
                for (int e = 0; e < VE; ++e) wv[e] = (float)t[e];
            } else {
                const f32x4 t = *reinterpret_cast<const f32x4*>(w + (size_t)n * K + k);
#pragma unroll
                for (int e = 0; e < VE; ++e) wv[e] = t[e];
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r0 + r < rows) {
                    const float* xr = x + (size_t)(r0 + r) * ldx + k;
#pragma unroll
                    for (int e = 0; e < VE; ++e) {
                        float xv = xr[e];
                        if (silu_in) xv = silu_f(xv);
                        acc[r] += xv * wv[e];
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float s = wsum(acc[r]);
            if (lane == 0 && r0 + r < rows) y[(size_t)(r0 + r) * ldy + n] = s + (bias ? bias[n] : 0.f);
        }
    }
}

// One row (a scalar timestep: every sample shares the embedding), bf16 weights, K <= 2048: the stack of all per-block time
// projections is a 50 MB weight stream.  act(x) is computed once per workgroup into LDS (not once per wave and k), a wave owns
// TWO output columns and issues every weight load of both before the first use, so the pass runs at bandwidth, not latency.
__global__ __launch_bounds__(256) void gemv_row1_kernel(const float* __restrict__ x, const bf16* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int N, int K, int silu_in) {
    __shared__ __attribute__((aligned(16))) float xs[2048];
    for (int k = threadIdx.x; k < K; k += 256) {
        const float v = x[k];
        xs[k] = silu_in ? silu_f(v) : v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
    if (n0 >= N) return;
    const int n1 = min(n0 + 1, N - 1);
    bf16x8 wa[4], wb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane * 8 + j * 512;
        if (k < K) {
            wa[j] = *reinterpret_cast<const bf16x8*>(w + (size_t)n0 * K + k);
            wb[j] = *reinterpret_cast<const bf16x8*>(w + (size_t)n1 * K + k);
        }
    }
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane * 8 + j * 512;
        if (k < K) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(xs + k), hi = *reinterpret_cast<const f32x4*>(xs + k + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a += lo[e] * (float)wa[j][e] + hi[e] * (float)wa[j][4 + e];
                b += lo[e] * (float)wb[j][e] + hi[e] * (float)wb[j][4 + e];
            }
        }
    }
    a = wsum(a);
    b = wsum(b);
    if (lane == 0) {
        y[n0] = a + (bias ? bias[n0] : 0.f);
        if (n0 + 1 < N) y[n0 + 1] = b + (bias ? bias[n0 + 1] : 0.f);
    }
}

// Several rows (per-sample timesteps: rows = batch): the same product on the matrix cores.  A wave owns 16 output
// columns; per 32-deep k step it streams one W fragment (16 n x 32 k, 16 B per lane) and builds NB x fragments
// (16 rows x 32 k) from the tiny L2-resident f32 input, applying SiLU and rounding to bf16 on the way.
template <int NB>
__global__ __launch_bounds__(256) void gemv_rows_mfma_kernel(const float* __restrict__ x, int ldx, const bf16* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y, int ldy, int rows,
                                                             int N, int K, int silu_in) {
    const int lane = threadIdx.x & 63;
    const int fr = lane & 15, fg = lane >> 4;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (n0 >= N) return;
    const bf16* wr = w + (size_t)min(n0 + fr, N - 1) * K + fg * 8;
    const float* xr[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) xr[b] = x + (size_t)min(b * 16 + fr, rows - 1) * ldx + fg * 8;
    f32x4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 32) {
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wr + k);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(xr[b] + k);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(xr[b] + k + 4);
            bf16x8 xf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xf[e] = (bf16)(silu_in ? silu_f(lo[e]) : lo[e]);
                xf[4 + e] = (bf16)(silu_in ? silu_f(hi[e]) : hi[e]);
            }
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[b], 0, 0, 0);  // D[n = 4fg + r][row = fr]
        }
    }
    const int n = n0 + fg * 4;
    if (n >= N) return;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + n);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int row = b * 16 + fr;
        if (row < rows) *reinterpret_cast<f32x4*>(y + (size_t)row * ldy + n) = acc[b] + bv;
    }
}

template <typename T>
int launch_gemv_rows(const float* x, int ldx, const void* w, const float* bias, float* y, int ldy, int rows, int N,
                     int K, int silu_in, hipStream_t st, int f32_inputs) {
    MRISR_REQUIRE(K % (16 / (int)sizeof(T)) == 0, "gemv K alignment");
    const dim3 grid((N + 3) / 4);
    ProfScope ps("time_embed_gemv", 2.0 * rows * (double)N * K, (double)N * K * sizeof(T), st);
    // (f32_inputs: the caller wants the one-row kernel's arithmetic - f32 inputs against bf16 weights, f32 sums - for many rows: the matrix-core
    // form below rounds the inputs to bf16)
    if (sizeof(T) == 2 && !f32_inputs && rows > 1 && rows <= 64 && K % 32 == 0 && N % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0) {
        const dim3 g2((N + 63) / 64);
        const bf16* wp = reinterpret_cast<const bf16*>(w);
        if (rows <= 16) hipLaunchKernelGGL((gemv_rows_mfma_kernel<1>), g2, dim3(256), 0, st, x, ldx, wp, bias, y, ldy, rows, N, K, silu_in);
        else if (rows <= 32) hipLaunchKernelGGL((gemv_rows_mfma_kernel<2>), g2, dim3(256), 0, st, x, ldx, wp, bias, y, ldy, rows, N, K, silu_in);
        else if (rows <= 48) hipLaunchKernelGGL((gemv_rows_mfma_kernel<3>), g2, dim3(256), 0, st, x, ldx, wp, bias, y, ldy, rows, N, K, silu_in);
        else hipLaunchKernelGGL((gemv_rows_mfma_kernel<4>), g2, dim3(256), 0, st, x, ldx, wp, bias, y, ldy, rows, N, K, silu_in);
        MRISR_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (sizeof(T) == 2 && rows == 1 && K % 8 == 0 && K <= 2048) {
        hipLaunchKernelGGL(gemv_row1_kernel, dim3((N + 7) / 8), dim3(256), 0, st, x, reinterpret_cast<const bf16*>(w), bias, y, N, K, silu_in);
        MRISR_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (rows <= 1)
        hipLaunchKernelGGL((gemv_rows_kernel<T, 1>), grid, dim3(256), 0, st, x, ldx, reinterpret_cast<const T*>(w), bias,
                           y, ldy, rows, N, K, silu_in);
    else
        hipLaunchKernelGGL((gemv_rows_kernel<T, 8>), grid, dim3(256), 0, st, x, ldx, reinterpret_cast<const T*>(w), bias,
                           y, ldy, rows, N, K, silu_in);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// z[m][q] = sum_k x[m][k] * A[q][k]: one wave per row m, lanes stride over 16-byte chunks of k; A (R x K, a few KB)
// stays in L1/L2.  Reads x exactly once: bandwidth-bound, ~5 us for 32768 x 320 bf16.
template <typename T, int RMAX>
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ A,
                                                        float* __restrict__ z, int M, int K, int R) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    float acc[RMAX];
#pragma unroll
    for (int q = 0; q < RMAX; ++q) acc[q] = 0.f;
    for (int k = lane * VE; k < K; k += 64 * VE) {
        float xv[VE];
        if constexpr (sizeof(T) == 2) {
            const bf16x8 t = *reinterpret_cast<const bf16x8*>(x + (size_t)m * ldx + k);
#pragma unroll
            for (int e = 0; e < VE; ++e) xv[e] = (float)t[e];
        } else {
            const f32x4 t = *reinterpret_cast<const f32x4*>(x + (size_t)m * ldx + k);
#pragma unroll
            for (int e = 0; e < VE; ++e) xv[e] = t[e];
        }
#pragma unroll
        for (int q = 0; q < RMAX; ++q) {
            if (q < R) {
                if constexpr (sizeof(T) == 2) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(A + (size_t)q * K + k);
#pragma unroll
                    for (int e = 0; e < VE; ++e) acc[q] += xv[e] * (float)a[e];
                } else {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(A + (size_t)q * K + k);
#pragma unroll
                    for (int e = 0; e < VE; ++e) acc[q] += xv[e] * a[e];
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RMAX; ++q) {
        if (q < R) {
            const float s = wsum(acc[q]);
            if (lane == 0) z[(size_t)m * R + q] = s;
        }
    }
}
// bf16 fast path: the same product on the matrix cores, no LDS and no cross-lane reduction.  A wave owns 16 rows:
// per 32-deep k step it loads one x fragment (16 rows x 32 k) and NQ adapter fragments (16 q x 32 k) straight from
// global/L1 into MFMA operand layout; D[row][q] accumulates in registers.
template <int NQ>
__global__ __launch_bounds__(256) void lora_down_mfma_kernel(const bf16* __restrict__ x, int ldx,
                                                             const bf16* __restrict__ A, float* __restrict__ z, int M,
                                                             int K, int R) {
    const int lane = threadIdx.x & 63;
    const int fr = lane & 15, fg = lane >> 4;
    const int m0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (m0 >= M) return;
    const bf16* xr = x + (size_t)min(m0 + fr, M - 1) * ldx + fg * 8;
    const bf16* ar[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) ar[b] = A + (size_t)min(b * 16 + fr, R - 1) * K + fg * 8;
    f32x4 acc[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 32) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xr + k);
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(ar[b] + k);
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, af, acc[b], 0, 0, 0);  // D[row = 4fg+r][q = fr]
        }
    }
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
        const int q = b * 16 + fr;
        if (q < R) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + fg * 4 + r;
                if (m < M) z[(size_t)m * R + q] = acc[b][r];
            }
        }
    }
}

template <typename T>
int launch_lora_down(const void* x, int ldx, const void* A, float* z, int M, int K, int R, hipStream_t st) {
    if (sizeof(T) == 2 && K % 32 == 0 && R <= 48) {
        ProfScope ps("lora_down", 2.0 * M * (double)R * K, (double)M * K * 2.0, st);
        const dim3 grid((M + 63) / 64);
        const bf16* xp = reinterpret_cast<const bf16*>(x);
        const bf16* ap = reinterpret_cast<const bf16*>(A);
        if (R <= 16) hipLaunchKernelGGL((lora_down_mfma_kernel<1>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
        else if (R <= 32) hipLaunchKernelGGL((lora_down_mfma_kernel<2>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
        else hipLaunchKernelGGL((lora_down_mfma_kernel<3>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
        MRISR_CHECK_HIP(hipGetLastError());
        return 0;
    }
    MRISR_REQUIRE(K % (16 / (int)sizeof(T)) == 0 && R >= 1 && R <= 48, "lora_down: K alignment / rank");
    ProfScope ps("lora_down", 2.0 * M * (double)R * K, (double)M * K * sizeof(T), st);
    const dim3 grid((M + 3) / 4);
    const T* xp = reinterpret_cast<const T*>(x);
    const T* ap = reinterpret_cast<const T*>(A);
    if (R <= 4) hipLaunchKernelGGL((lora_down_kernel<T, 4>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
    else if (R <= 8) hipLaunchKernelGGL((lora_down_kernel<T, 8>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
    else if (R <= 12) hipLaunchKernelGGL((lora_down_kernel<T, 12>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
    else if (R <= 24) hipLaunchKernelGGL((lora_down_kernel<T, 24>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
    else hipLaunchKernelGGL((lora_down_kernel<T, 48>), grid, dim3(256), 0, st, xp, ldx, ap, z, M, K, R);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ void timestep_embedding_kernel(const long long* __restrict__ t, int t_is_scalar, float* __restrict__ out,
                                          int rows, int dim) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * half) return;
    const int r = i / half, j = i - r * half;
    const float tv = (float)(t_is_scalar ? t[0] : t[r]);
    const float freq = expf(-9.210340371976184f * (float)j / (float)half);  // ln(10000)
    const float ang = tv * freq;
    out[(size_t)r * dim + j] = cosf(ang);
    out[(size_t)r * dim + half + j] = sinf(ang);
}
int launch_timestep_embedding(const long long* t, int t_is_scalar, float* out, int rows, int dim, hipStream_t st) {
    const int n = rows * (dim / 2);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t, t_is_scalar, out, rows, dim);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// direct convolution, one thread per (output pixel, output channel); f32 accumulate.
// Only for the few layers whose channel counts are far below one MFMA K tile.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void direct_conv_kernel(const DirectConvArgs a) {
    const long long total = (long long)a.B * a.Hout * a.Wout * a.Cout;
    const T* x = reinterpret_cast<const T*>(a.x);
    const T* w = reinterpret_cast<const T*>(a.w);
    T* y = reinterpret_cast<T*>(a.y);
    const int Kt = a.ks * a.ks * a.Cin;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int n = (int)(i % a.Cout);
        const long long m = i / a.Cout;
        const int ox = (int)(m % a.Wout);
        const int oy = (int)((m / a.Wout) % a.Hout);
        const int b = (int)(m / ((long long)a.Wout * a.Hout));
        float acc = a.bias ? a.bias[n] : 0.f;
        for (int ky = 0; ky < a.ks; ++ky) {
            const int iy = oy * a.stride + ky - a.pad;
            if (iy < 0 || iy >= a.Hin) continue;
            for (int kx = 0; kx < a.ks; ++kx) {
                const int ix = ox * a.stride + kx - a.pad;
                if (ix < 0 || ix >= a.Win) continue;
                const T* xp = x + (((size_t)b * a.Hin + iy) * a.Win + ix) * a.Cin;
                const T* wp = w + (size_t)n * Kt + (ky * a.ks + kx) * a.Cin;
                for (int c = 0; c < a.Cin; ++c) acc += to_f32(xp[c]) * to_f32(wp[c]);
            }
        }
        if (a.act == ACT_SILU) acc = silu_f(acc);
        else if (a.act == ACT_RELU) acc = fmaxf(acc, 0.f);
        if (a.add) acc += to_f32(reinterpret_cast<const T*>(a.add)[i]);
        y[i] = from_f32<T>(acc);
    }
}
// Small-fan-in convolution (conv_in: 3x3x4 = 36 taps): the transposed filter bank [tap*Cin][Cout] sits in LDS, a
// thread produces 8 consecutive output channels of one pixel, so x is read once per pixel-thread-group (broadcast
// within the wave), filters come as 16-byte LDS vectors and the store is one 16/32-byte vector per thread.
template <typename T>
__global__ __launch_bounds__(256) void small_conv_kernel(const DirectConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sm_raw[];
    T* wT = reinterpret_cast<T*>(sm_raw);
    const T* x = reinterpret_cast<const T*>(a.x);
    const T* w = reinterpret_cast<const T*>(a.w);
    T* y = reinterpret_cast<T*>(a.y);
    const int Kt = a.ks * a.ks * a.Cin;
    for (int i = threadIdx.x; i < Kt * a.Cout; i += 256) {
        const int k = i / a.Cout, n = i - k * a.Cout;
        wT[i] = w[(size_t)n * Kt + k];
    }
    __syncthreads();
    const int CG = a.Cout / 8;
    const long long items = (long long)a.B * a.Hout * a.Wout * CG;
    for (long long it = blockIdx.x * 256ll + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
        const int cg = (int)(it % CG);
        const long long m = it / CG;
        const int ox = (int)(m % a.Wout);
        const int oy = (int)((m / a.Wout) % a.Hout);
        const int b = (int)(m / ((long long)a.Wout * a.Hout));
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = a.bias ? a.bias[cg * 8 + e] : 0.f;
        for (int ky = 0; ky < a.ks; ++ky) {
            const int iy = oy * a.stride + ky - a.pad;
            if (iy < 0 || iy >= a.Hin) continue;
            for (int kx = 0; kx < a.ks; ++kx) {
                const int ix = ox * a.stride + kx - a.pad;
                if (ix < 0 || ix >= a.Win) continue;
                const T* xp = x + (((size_t)b * a.Hin + iy) * a.Win + ix) * a.Cin;
                const T* wr = wT + (size_t)((ky * a.ks + kx) * a.Cin) * a.Cout + cg * 8;
                float xin[4];
                const bool vec4 = sizeof(T) == 2 && a.Cin == 4;  // conv_in: the pixel's 4 channels in one 8-byte load
                if constexpr (sizeof(T) == 2) {
                    if (vec4) {
                        const bf16x4 t = *reinterpret_cast<const bf16x4*>(xp);
                        xin[0] = (float)t[0]; xin[1] = (float)t[1]; xin[2] = (float)t[2]; xin[3] = (float)t[3];
                    }
                }
                for (int c = 0; c < a.Cin; ++c) {
                    const float xv = vec4 ? xin[c & 3] : to_f32(xp[c]);
                    if constexpr (sizeof(T) == 2) {  // one 16-byte LDS read for the 8 output channels
                        const bf16x8 w8 = *reinterpret_cast<const bf16x8*>(wr + (size_t)c * a.Cout);
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[e] += xv * (float)w8[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[e] += xv * to_f32(wr[(size_t)c * a.Cout + e]);
                    }
                }
            }
        }
        const size_t o = (size_t)m * a.Cout + cg * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = acc[e];
            if (a.act == ACT_SILU) v = silu_f(v);
            else if (a.act == ACT_RELU) v = fmaxf(v, 0.f);
            if (a.add) v += to_f32(reinterpret_cast<const T*>(a.add)[o + e]);
            acc[e] = v;
        }
        if constexpr (sizeof(T) == 2) {
            bf16x8 ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = (bf16)acc[e];
            *reinterpret_cast<bf16x8*>(y + o) = ov;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) y[o + e] = acc[e];
        }
    }
}

// conv_in on the matrix cores (bf16, 3x3, 4 input channels, stride 1, pad 1): K = 36 padded to 64 = two MFMA steps.  The filter
// bank sits in LDS as [Cout][40] (taps 0-7 | tap 8 + zeros), a wave takes 16 consecutive pixels, gathers their 3x3x4
// neighbourhoods straight into the row fragments (one 8-byte load per tap), runs Cout/16 x 2 MFMAs and leaves through a
// per-wave LDS tile so that the 16 x Cout outputs - one contiguous run in NHWC - are written as 16-byte pieces.
__global__ __launch_bounds__(256) void conv_in_mfma_kernel(const DirectConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sm_raw[];
    bf16* wl = reinterpret_cast<bf16*>(sm_raw);                                  // [Cout][40]
    const int OP = a.Cout + 8;
    bf16* ot = wl + (size_t)a.Cout * 40 + (size_t)(threadIdx.x >> 6) * 16 * OP;  // this wave's [16][Cout + 8]
    float* bl = reinterpret_cast<float*>(wl + (size_t)a.Cout * 40 + (size_t)4 * 16 * OP);  // [Cout] bias
    const bf16* x = reinterpret_cast<const bf16*>(a.x);
    const bf16* w = reinterpret_cast<const bf16*>(a.w);
    bf16* y = reinterpret_cast<bf16*>(a.y);
    for (int i = threadIdx.x; i < a.Cout * 10; i += 256) {  // 72-byte filter rows -> 80-byte LDS rows, 8 bytes at a time
        const int n = i / 10, j = i - n * 10;
        const uint2 v = j < 9 ? *reinterpret_cast<const uint2*>(w + (size_t)n * 36 + j * 4) : make_uint2(0u, 0u);
        *reinterpret_cast<uint2*>(wl + (size_t)n * 40 + j * 4) = v;
    }
    for (int i = threadIdx.x; i < a.Cout; i += 256) bl[i] = a.bias ? a.bias[i] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, fr = lane & 15, fg = lane >> 4;
    const int M = a.B * a.Hout * a.Wout;  // < 2^31 (checked by the launcher)
    const int ngroups = (M + 15) / 16;
    const int NFR = a.Cout / 16, CPR = a.Cout / 8;
    for (int pg = blockIdx.x * 4 + (threadIdx.x >> 6); pg < ngroups; pg += gridDim.x * 4) {
        const int m = pg * 16 + fr;
        bf16x8 af0 = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}, af1 = af0;
        if (m < M) {
            const int ox = m % a.Wout, oy = (m / a.Wout) % a.Hout, b = m / (a.Wout * a.Hout);
            auto tap4 = [&](int t) -> uint2 {  // the 4 channels of the pixel under tap t (zeros outside the image)
                const int ky = t / 3, kx = t - ky * 3;
                const int iy = oy + ky - 1, ix = ox + kx - 1;
                if (iy < 0 || iy >= a.Hin || ix < 0 || ix >= a.Win) return make_uint2(0u, 0u);
                return *reinterpret_cast<const uint2*>(x + (((size_t)b * a.Hin + iy) * a.Win + ix) * 4);
            };
            const uint2 p0 = tap4(fg * 2), p1 = tap4(fg * 2 + 1);
            af0 = __builtin_bit_cast(bf16x8, make_uint4(p0.x, p0.y, p1.x, p1.y));
            if (fg == 0) {
                const uint2 p8 = tap4(8);
                af1 = __builtin_bit_cast(bf16x8, make_uint4(p8.x, p8.y, 0u, 0u));
            }
        }
        for (int i = 0; i < NFR; ++i) {
            const bf16* wr = wl + (size_t)(i * 16 + fr) * 40;
            const bf16x8 wf0 = *reinterpret_cast<const bf16x8*>(wr + fg * 8);
            bf16x8 wf1 = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (fg == 0) wf1 = *reinterpret_cast<const bf16x8*>(wr + 32);
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0, af0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1, af1, acc, 0, 0, 0);
            const int n = i * 16 + fg * 4;
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bl + n);
            // `add` joins in f32, before the one rounding (as the GEMM epilogue's residual does): rounding the conv first and the sum
            // again costs up to a bf16 ulp of the larger term
            bf16x4 ad = bf16x4{0, 0, 0, 0};
            if (a.add && m < M) ad = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(a.add) + (size_t)m * a.Cout + n);
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[r] + b4[r];
                if (a.act == ACT_SILU) v = silu_f(v);
                else if (a.act == ACT_RELU) v = fmaxf(v, 0.f);
                o[r] = (bf16)(v + (float)ad[r]);
            }
            *reinterpret_cast<bf16x4*>(ot + fr * OP + n) = o;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own LDS writes (no other wave touches this tile)
        __builtin_amdgcn_wave_barrier();
        for (int c = lane; c < 16 * CPR; c += 64) {
            const int row = c / CPR, col = (c - row * CPR) * 8;
            const int mo = pg * 16 + row;
            if (mo >= M) continue;
            *reinterpret_cast<bf16x8*>(y + (size_t)mo * a.Cout + col) = *reinterpret_cast<const bf16x8*>(ot + row * OP + col);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // tile reads done before the next group overwrites it
        __builtin_amdgcn_wave_barrier();
    }
}

// launch attributes (called from gemm_prepare, i.e. before any graph capture)
int direct_conv_prepare() {
    static bool done = false;
    if (!done) {
        MRISR_CHECK_HIP(hipFuncSetAttribute((const void*)conv_in_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        done = true;
    }
    return 0;
}

template <typename T>
int launch_direct_conv(const DirectConvArgs& a, hipStream_t st) {
    const size_t wbytes = (size_t)a.ks * a.ks * a.Cin * a.Cout * sizeof(T);
    if (sizeof(T) == 2 && a.ks == 3 && a.Cin == 4 && a.stride == 1 && a.pad == 1 && a.Cout % 16 == 0 && a.Hout == a.Hin && a.Wout == a.Win) {
        const size_t smem = ((size_t)a.Cout * 40 + (size_t)4 * 16 * (a.Cout + 8)) * 2 + (size_t)a.Cout * 4;
        if (smem <= 80 * 1024 && (long long)a.B * a.Hout * a.Wout * a.Cout < (1ll << 31)) {  // Cout <= 384: two workgroups per CU
            if (direct_conv_prepare()) return 1;
            const long long M = (long long)a.B * a.Hout * a.Wout;
            long long blocks = ((M + 15) / 16 + 3) / 4;
            if (blocks > 256) blocks = 256;  // every workgroup first stages the filter bank
            ProfScope ps("conv_in_mfma", 2.0 * M * a.Cout * 36, 2.0 * (M * 4.0 + (double)M * a.Cout), st);
            hipLaunchKernelGGL(conv_in_mfma_kernel, dim3((unsigned)blocks), dim3(256), smem, st, a);
            MRISR_CHECK_HIP(hipGetLastError());
            return 0;
        }
    }
    if (a.Cout % 8 == 0 && wbytes <= 48 * 1024) {
        const long long items = (long long)a.B * a.Hout * a.Wout * (a.Cout / 8);
        long long blocks = (items + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        ProfScope ps("small_conv", 2.0 * items * 8 * a.ks * a.ks * a.Cin,
                     sizeof(T) * ((double)a.B * a.Hin * a.Win * a.Cin + (double)items * 8), st);
        hipLaunchKernelGGL(small_conv_kernel<T>, dim3((unsigned)blocks), dim3(256), wbytes, st, a);
        MRISR_CHECK_HIP(hipGetLastError());
        return 0;
    }
    const long long total = (long long)a.B * a.Hout * a.Wout * a.Cout;
    long long blocks = (total + 255) / 256;
    if (blocks > 65535 * 4) blocks = 65535 * 4;
    ProfScope ps("direct_conv", 2.0 * total * a.ks * a.ks * a.Cin,
                 sizeof(T) * ((double)a.B * a.Hin * a.Win * a.Cin + (double)total), st);
    hipLaunchKernelGGL(direct_conv_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// conv_out-style reduction: few output channels (<= 8), deep K: one wave per output pixel.
// (used through launch_direct_conv's sibling below when Cout <= 8 and Cin % 64 == 0)

// ------------------------------------------------------------------------------------------------
// boundary layout/dtype conversion
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float load_any(const void* p, int dt, size_t i) {
    switch (dt) {
        case DT_F32: return reinterpret_cast<const float*>(p)[i];
        case DT_BF16: return (float)reinterpret_cast<const bf16*>(p)[i];
        default: return (float)reinterpret_cast<const _Float16*>(p)[i];
    }
}
__device__ __forceinline__ void store_any(void* p, int dt, size_t i, float v) {
    switch (dt) {
        case DT_F32: reinterpret_cast<float*>(p)[i] = v; break;
        case DT_BF16: reinterpret_cast<bf16*>(p)[i] = (bf16)v; break;
        default: reinterpret_cast<_Float16*>(p)[i] = (_Float16)v; break;
    }
}

template <typename T>
__global__ void nchw_to_nhwc_kernel(const void* src, int sdt, T* dst, int B, int C, int H, int W) {
    const long long total = (long long)B * C * H * W;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long p = i / C;  // b*H*W + y*W + x
        const long long hw = (long long)H * W;
        const long long b = p / hw, r = p - b * hw;
        dst[i] = from_f32<T>(load_any(src, sdt, (size_t)((b * C + c) * hw + r)));
    }
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* src, void* dst, int ddt, int B, int C, int H, int W, float scale) {
    const long long total = (long long)B * C * H * W;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        // i indexes the NCHW destination (coalesced writes)
        const long long hw = (long long)H * W;
        const long long r = i % hw;
        const long long bc = i / hw;
        const long long c = bc % C, b = bc / C;
        store_any(dst, ddt, (size_t)i, scale * to_f32(src[(size_t)((b * hw + r) * C + c)]));
    }
}
static inline unsigned nblocks(long long total) {
    long long b = (total + 255) / 256;
    return (unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}
template <typename T>
int launch_nchw_to_nhwc(const void* src, int src_dtype, void* dst, int B, int C, int H, int W, hipStream_t st) {
    ProfScope ps("layout_convert", 0.0, (double)B * C * H * W * (sizeof(T) + 4.0), st);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, dim3(nblocks((long long)B * C * H * W)), dim3(256), 0, st, src,
                       src_dtype, reinterpret_cast<T*>(dst), B, C, H, W);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template <typename T>
int launch_nhwc_to_nchw(const void* src, void* dst, int dst_dtype, int B, int C, int H, int W, float scale,
                        hipStream_t st) {
    ProfScope ps("layout_convert", 0.0, (double)B * C * H * W * (sizeof(T) + 4.0), st);
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, dim3(nblocks((long long)B * C * H * W)), dim3(256), 0, st,
                       reinterpret_cast<const T*>(src), dst, dst_dtype, B, C, H, W, scale);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
__global__ void add_inplace_kernel(T* x, const T* y, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        x[i] = from_f32<T>(to_f32(x[i]) + to_f32(y[i]));
}
template <typename T>
int launch_add_inplace(void* x, const void* y, long long n, hipStream_t st) {
    ProfScope ps("residual_add", 0.0, 3.0 * n * sizeof(T), st);
    hipLaunchKernelGGL(add_inplace_kernel<T>, dim3(nblocks(n)), dim3(256), 0, st, reinterpret_cast<T*>(x),
                       reinterpret_cast<const T*>(y), n);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// PixelUnshuffle(r) of an NCHW image straight into NHWC:  out[b][y][x][c*r*r + dy*r + dx] = in[b][c][y*r+dy][x*r+dx]
template <typename T>
__global__ void pixel_unshuffle_kernel(const void* src, int sdt, T* dst, int B, int C, int H, int W, int r) {
    const int Ho = H / r, Wo = W / r, Co = C * r * r;
    const long long total = (long long)B * Ho * Wo * Co;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int co = (int)(i % Co);
        const long long p = i / Co;
        const int x = (int)(p % Wo);
        const int y = (int)((p / Wo) % Ho);
        const int b = (int)(p / ((long long)Wo * Ho));
        const int c = co / (r * r), dy = (co / r) % r, dx = co % r;
        dst[i] = from_f32<T>(load_any(src, sdt, (((size_t)b * C + c) * H + (y * r + dy)) * W + (x * r + dx)));
    }
}
template <typename T>
int launch_pixel_unshuffle_nchw(const void* src, int src_dtype, void* dst, int B, int C, int H, int W, int r,
                                hipStream_t st) {
    hipLaunchKernelGGL(pixel_unshuffle_kernel<T>, dim3(nblocks((long long)B * C * H * W)), dim3(256), 0, st, src,
                       src_dtype, reinterpret_cast<T*>(dst), B, C, H, W, r);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// weight packers (load time)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void pack_rows_kernel(const float* src, int rows, int cols, T* dst, int ld_dst, int row_off, int col_off,
                                 int row_map, int half, float scale) {
    const long long total = (long long)rows * cols;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (long long)r * cols);
        int dr = r + row_off;
        if (row_map == 1) {  // GEGLU: src rows [0,half) = u, [half,2half) = gate -> blocks of 16 interleaved
            const int isg = r >= half;
            const int j = isg ? r - half : r;
            dr = (j >> 4) * 32 + (j & 15) + (isg ? 16 : 0) + row_off;
        }
        dst[(size_t)dr * ld_dst + col_off + c] = from_f32<T>(scale * src[i]);
    }
}
template <typename T>
int launch_pack_rows(const float* src, int rows, int cols, void* dst, int ld_dst, int row_off, int col_off,
                     int row_map, int half, float scale, hipStream_t st) {
    hipLaunchKernelGGL(pack_rows_kernel<T>, dim3(nblocks((long long)rows * cols)), dim3(256), 0, st, src, rows, cols,
                       reinterpret_cast<T*>(dst), ld_dst, row_off, col_off, row_map, half, scale);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template <typename T>
__global__ void pack_conv_kernel(const float* src, T* dst, int Cout, int Cin, int ks) {
    const long long total = (long long)Cout * Cin * ks * ks;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        // i indexes dst [Cout][ky][kx][Cin]
        const int c = (int)(i % Cin);
        const long long t = i / Cin;
        const int tap = (int)(t % (ks * ks));
        const int n = (int)(t / (ks * ks));
        dst[i] = from_f32<T>(src[((size_t)n * Cin + c) * ks * ks + tap]);
    }
}
// the same filter bank with both channel counts padded up (zeros): dst [Cout_pad][ky][kx][Cin_pad]
template <typename T>
__global__ void pack_conv_padded_kernel(const float* src, T* dst, int Cout, int Cin, int ks, int Cout_pad, int Cin_pad) {
    const long long total = (long long)Cout_pad * Cin_pad * ks * ks;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % Cin_pad);
        const long long t = i / Cin_pad;
        const int tap = (int)(t % (ks * ks));
        const int n = (int)(t / (ks * ks));
        dst[i] = from_f32<T>(n < Cout && c < Cin ? src[((size_t)n * Cin + c) * ks * ks + tap] : 0.f);
    }
}
template <typename T>
int launch_pack_conv3x3_padded(const float* src, void* dst, int Cout, int Cin, int ks, int Cout_pad, int Cin_pad, hipStream_t st) {
    hipLaunchKernelGGL(pack_conv_padded_kernel<T>, dim3(nblocks((long long)Cout_pad * Cin_pad * ks * ks)), dim3(256), 0, st, src,
                       reinterpret_cast<T*>(dst), Cout, Cin, ks, Cout_pad, Cin_pad);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template <typename T>
int launch_pack_conv3x3(const float* src, void* dst, int Cout, int Cin, int ks, hipStream_t st) {
    hipLaunchKernelGGL(pack_conv_kernel<T>, dim3(nblocks((long long)Cout * Cin * ks * ks)), dim3(256), 0, st, src,
                       reinterpret_cast<T*>(dst), Cout, Cin, ks);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
// ---- sub-pixel decomposition of `nearest x2 -> conv3x3` -----------------------------------------------------------------------
// Output pixel (2y + py, 2x + px) reads the up-sampled rows 2y + py + dy, dy = -1, 0, 1, i.e. the low-resolution rows
//   py = 0:  y - 1 (dy = -1),  y (dy = 0, +1)            py = 1:  y (dy = -1, 0),  y + 1 (dy = +1)
// (zero padding of the up-sampled image = out-of-range low-resolution rows, exactly) - a 2 x 2 window starting at y - 1 + py whose
// tap t = 0 / 1 carries the sum of the 3 x 3 taps {0} / {1, 2} (py = 0) or {0, 1} / {2} (py = 1); the same along x.  4/9 of the MACs.
template <typename T>
__global__ void pack_conv_subpix_kernel(const float* __restrict__ src, T* __restrict__ dst, int Cout, int Cin) {
    const long long per = (long long)Cout * 4 * Cin;  // one parity's bank [Cout][2][2][Cin]
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < 4 * per; i += (long long)gridDim.x * 256) {
        const int par = (int)(i / per);
        const long long j = i - par * per;
        const int c = (int)(j % Cin);
        const int t = (int)((j / Cin) % 4);
        const int n = (int)(j / (4ll * Cin));
        const int py = par >> 1, px = par & 1, ty = t >> 1, tx = t & 1;
        // 3 x 3 taps folded into low-resolution tap (ty, tx): k0 .. k1 inclusive
        const int ky0 = py == 0 ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), ky1 = py == 0 ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
        const int kx0 = px == 0 ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kx1 = px == 0 ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
        float acc = 0.f;
        for (int ky = ky0; ky <= ky1; ++ky)
            for (int kx = kx0; kx <= kx1; ++kx) acc += src[((size_t)n * Cin + c) * 9 + ky * 3 + kx];
        dst[i] = from_f32<T>(acc);
    }
}
template <typename T>
int launch_pack_conv_subpix(const float* src, void* dst, int Cout, int Cin, hipStream_t st) {
    hipLaunchKernelGGL(pack_conv_subpix_kernel<T>, dim3(nblocks(16ll * Cout * Cin)), dim3(256), 0, st, src, reinterpret_cast<T*>(dst), Cout, Cin);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
// planes [4][B][H][W][C] (parity-major) -> out [B][2H][2W][C]; 16-byte pieces, one output pixel row of C channels per group of C/8 threads
template <typename T>
__global__ void subpix_shuffle_kernel(const T* __restrict__ planes, T* __restrict__ out, int B, int H, int W, int C) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int cv = C / VE;
    const long long total = (long long)B * 4 * H * W * cv;
    const long long plane = (long long)B * H * W * C;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int v = (int)(i % cv);
        long long p = i / cv;                 // output pixel index (b, Y, X)
        const int X = (int)(p % (2 * W)); p /= 2 * W;
        const int Y = (int)(p % (2 * H));
        const int b = (int)(p / (2 * H));
        const int par = (Y & 1) * 2 + (X & 1);
        const long long src = par * plane + (((long long)b * H + (Y >> 1)) * W + (X >> 1)) * C + (long long)v * VE;
        *reinterpret_cast<uint4*>(out + i * VE) = *reinterpret_cast<const uint4*>(planes + src);
    }
}
template <typename T>
int launch_subpix_shuffle(const void* planes, void* out, int B, int H, int W, int C, hipStream_t st) {
    MRISR_REQUIRE(C % (16 / (int)sizeof(T)) == 0, "sub-pixel shuffle: channel count must fill 16-byte pieces");
    ProfScope ps("subpix_shuffle", 0.0, 2.0 * 4.0 * B * H * W * C * sizeof(T), st);
    hipLaunchKernelGGL(subpix_shuffle_kernel<T>, dim3(nblocks(4ll * B * H * W * C / (16 / (int)sizeof(T)))), dim3(256), 0, st,
                       reinterpret_cast<const T*>(planes), reinterpret_cast<T*>(out), B, H, W, C);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
__global__ void pack_bias_geglu_kernel(const float* src, float* dst, int half) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= 2 * half) return;
    const int isg = r >= half;
    const int j = isg ? r - half : r;
    dst[(j >> 4) * 32 + (j & 15) + (isg ? 16 : 0)] = src[r];
}
int launch_pack_bias_geglu(const float* src, float* dst, int half, hipStream_t st) {
    hipLaunchKernelGGL(pack_bias_geglu_kernel, dim3((2 * half + 255) / 256), dim3(256), 0, st, src, dst, half);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
// ---- ff.net.2 composed with proj_out (runner.h::transformer): W'[n][k] = sum_j Wp[n][j] W2[j][k] and b'[n] = sum_j Wp[n][j] b2[j] + bp[n],
// both in f32 from the f32 masters (j ascending), W' rounded once to bf16.  64 x 64 output tiles, 16 values of j per LDS stage.
__global__ void __launch_bounds__(256) compose_ff_proj_kernel(const float* __restrict__ wp, const float* __restrict__ w2, bf16* __restrict__ dst,
                                                              int C, int K4, int ld_dst) {
    __shared__ float sa[16][64 + 1];  // Wp tile [j][n]
    __shared__ float sb[16][64];      // W2 tile [j][k]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int n0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
    float acc[4][4] = {};
    for (int j0 = 0; j0 < C; j0 += 16) {
        for (int i = threadIdx.x; i < 64 * 16; i += 256) {
            sa[i & 15][i >> 4] = wp[(size_t)(n0 + (i >> 4)) * C + j0 + (i & 15)];
            sb[i >> 6][i & 63] = w2[(size_t)(j0 + (i >> 6)) * K4 + k0 + (i & 63)];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = sa[j][ty * 4 + r]; b[r] = sb[j][tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += a[r] * b[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) dst[(size_t)(n0 + ty * 4 + r) * ld_dst + k0 + tx * 4 + c] = from_f32<bf16>(acc[r][c]);
}
__global__ void compose_ff_proj_bias_kernel(const float* __restrict__ wp, const float* __restrict__ b2, const float* __restrict__ bp,
                                            float* __restrict__ dst, int C) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= C) return;
    float acc = 0.f;
    if (b2)
        for (int j = 0; j < C; ++j) acc += wp[(size_t)n * C + j] * b2[j];
    dst[n] = acc + (bp ? bp[n] : 0.f);
}
int launch_compose_ff_proj(const float* wp, const float* w2, const float* b2, const float* bp, void* dst_bf16, int ld_dst, float* bias_dst,
                           int C, int K4, hipStream_t st) {
    MRISR_REQUIRE(wp && w2 && dst_bf16 && bias_dst && C > 0 && C % 64 == 0 && K4 > 0 && K4 % 64 == 0 && ld_dst >= K4,
                  "composed ff.net.2 / proj_out bank: widths that are multiples of 64");
    hipLaunchKernelGGL(compose_ff_proj_kernel, dim3(K4 / 64, C / 64), dim3(256), 0, st, wp, w2, reinterpret_cast<bf16*>(dst_bf16), C, K4, ld_dst);
    hipLaunchKernelGGL(compose_ff_proj_bias_kernel, dim3((C + 255) / 256), dim3(256), 0, st, wp, b2, bp, bias_dst, C);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template <typename T>
__global__ void scale_inplace_kernel(T* p, float s, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = from_f32<T>(to_f32(p[i]) * s);
}
template <typename T>
int launch_scale_inplace(void* p, float s, long long n, hipStream_t st) {
    hipLaunchKernelGGL(scale_inplace_kernel<T>, dim3(nblocks(n)), dim3(256), 0, st, reinterpret_cast<T*>(p), s, n);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template <typename T>
__global__ void fill_zero_kernel(T* p, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = from_f32<T>(0.f);
}
template <typename T>
int launch_fill_zero(void* p, long long n, hipStream_t st) {
    hipLaunchKernelGGL(fill_zero_kernel<T>, dim3(nblocks(n)), dim3(256), 0, st, reinterpret_cast<T*>(p), n);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void select_row_kernel(const float* __restrict__ table, const int* __restrict__ step, int first, float* __restrict__ out, int n) {
    const float* row = table + (size_t)(*step - first) * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = row[i];
}
int launch_select_row(const float* table, const int* step, int first, float* out, int n, hipStream_t st) {
    hipLaunchKernelGGL(select_row_kernel, dim3((n + 255) / 256), dim3(256), 0, st, table, step, first, out, n);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// fp8 (OCP e4m3) row quantisation of packed bf16 weights: one wave per row, scale = amax / 448 (BASELINE configs[4])
// ------------------------------------------------------------------------------------------------
__global__ void quant_rows_fp8_kernel(const bf16* __restrict__ src, int rows, int cols, unsigned char* __restrict__ dst, float* __restrict__ scales) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bf16* s = src + (size_t)row * cols;
    float am = 0.f;
    for (int c = lane; c < cols; c += 64) am = fmaxf(am, fabsf((float)s[c]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
    const float sc = fmaxf(am, 1e-20f) * (1.0f / 448.0f), inv = 1.0f / sc;
    if (lane == 0) scales[row] = sc;
    unsigned short* d = reinterpret_cast<unsigned short*>(dst + (size_t)row * cols);
    for (int c = lane * 2; c < cols; c += 128) {
        const int pk = __builtin_amdgcn_cvt_pk_fp8_f32((float)s[c] * inv, (float)s[c + 1] * inv, 0, false);
        d[c >> 1] = (unsigned short)(pk & 0xFFFF);
    }
}
int launch_quant_rows_fp8(const void* src_bf16, int rows, int cols, void* dst8, float* scales, hipStream_t st) {
    MRISR_REQUIRE(cols % 2 == 0, "fp8 row quantisation: even column count");
    hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, reinterpret_cast<const bf16*>(src_bf16), rows, cols,
                       reinterpret_cast<unsigned char*>(dst8), scales);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

#define INST(T)                                                                                                    \
    template int launch_gemv_rows<T>(const float*, int, const void*, const float*, float*, int, int, int, int, int, \
                                     hipStream_t, int);                                                            \
    template int launch_direct_conv<T>(const DirectConvArgs&, hipStream_t);                                        \
    template int launch_lora_down<T>(const void*, int, const void*, float*, int, int, int, hipStream_t);           \
    template int launch_nchw_to_nhwc<T>(const void*, int, void*, int, int, int, int, hipStream_t);                 \
    template int launch_nhwc_to_nchw<T>(const void*, void*, int, int, int, int, int, float, hipStream_t);          \
    template int launch_add_inplace<T>(void*, const void*, long long, hipStream_t);                                \
    template int launch_pixel_unshuffle_nchw<T>(const void*, int, void*, int, int, int, int, int, hipStream_t);    \
    template int launch_pack_rows<T>(const float*, int, int, void*, int, int, int, int, int, float, hipStream_t);  \
    template int launch_pack_conv3x3<T>(const float*, void*, int, int, int, hipStream_t);                          \
    template int launch_pack_conv3x3_padded<T>(const float*, void*, int, int, int, int, int, hipStream_t);         \
    template int launch_pack_conv_subpix<T>(const float*, void*, int, int, hipStream_t);                            \
    template int launch_subpix_shuffle<T>(const void*, void*, int, int, int, int, hipStream_t);                     \
    template int launch_scale_inplace<T>(void*, float, long long, hipStream_t);                                     \
    template int launch_fill_zero<T>(void*, long long, hipStream_t);
INST(float)
INST(bf16)

}  // namespace mrisr
