// DoRA (weight-decomposed LoRA, peft use_dora=True): the per-output-row magnitude of an adapted linear.
//
//   wn[j] = || W[j,:] + s (B A)[j,:] ||_2      g[j] = m[j] / wn[j]      y = b + g o (x W^T + s (x A^T) B^T)
//
// dora_scale      : g from the f32 masters, and the scaled rows the forward multiplies by - g W (un-merged: the adapter stays apart, its B
//                   rows scaled by dora_pack_b) or g (W + s B A) (merged)
// dora_pack_b     : g s B into an f32 [n][r] bank or into the sB columns of a [W | sB] weight
// dora_mag_grad   : d(loss)/dm from dY and the projection's own output, slab partials + an ordered reduce (no atomics: bits repeat)
#include "common.h"
#include "prof.h"

namespace mrisr {

namespace {
template <typename T> struct DVec;
template <> struct DVec<bf16> { static constexpr int N = 8; typedef bf16x8 type; };
template <> struct DVec<float> { static constexpr int N = 4; typedef f32x4 type; };

__device__ __forceinline__ float dora_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// raw row -> packed row of a GEGLU projection (half > 0), identity otherwise
__device__ __forceinline__ int geglu_packed_row_or_id(int raw, int half) { return half > 0 ? geglu_packed_row(raw, half) : raw; }
}  // namespace

// ---- dora_scale --------------------------------------------------------------------------------------------------------------------
// One workgroup per raw row j.  Pass 1: v[c] = W[j][c] + sum_q (s B[j][q]) A[q][c], sum of squares over c (per-lane partials, wave
// shuffle, four wave sums added in wave order: the same bits every launch).  Pass 2: out[dst(j)][c] = g (merged ? v[c] : W[j][c]).
template <typename T>
__global__ __launch_bounds__(256) void dora_scale_kernel(const float* __restrict__ W, const float* __restrict__ A, const float* __restrict__ B,
                                                         const float* __restrict__ mag, float s, float* __restrict__ g, T* __restrict__ out,
                                                         int ld, int row_off, int n, int k, int r, int half, int merged) {
    __shared__ float sb[128];
    __shared__ float wsum[4];
    const int j = blockIdx.x;
    if (j >= n) return;
    for (int q = threadIdx.x; q < r; q += 256) sb[q] = s * B[(size_t)j * r + q];
    __syncthreads();
    const float* wr = W + (size_t)j * k;
    float ss = 0.f;
    for (int c = threadIdx.x; c < k; c += 256) {
        float acc = 0.f;
        for (int q = 0; q < r; ++q) acc = fmaf(sb[q], A[(size_t)q * k + c], acc);
        const float v = wr[c] + acc;
        ss = fmaf(v, v, ss);
    }
    ss = dora_wsum(ss);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float gj = mag[j] / sqrtf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    const int dr = row_off + geglu_packed_row_or_id(j, half);
    if (threadIdx.x == 0) g[dr] = gj;
    if (!out) return;
    T* orow = out + (size_t)dr * ld;
    for (int c = threadIdx.x; c < k; c += 256) {
        float v = wr[c];
        if (merged) {
            float acc = 0.f;
            for (int q = 0; q < r; ++q) acc = fmaf(sb[q], A[(size_t)q * k + c], acc);
            v += acc;
        }
        orow[c] = from_f32<T>(gj * v);
    }
}

template <typename T>
int launch_dora_scale(const float* W, const float* A, const float* B, const float* mag, float s, float* g, void* out, int ld, int row_off, int n,
                      int k, int r, int geglu_half, int merged, hipStream_t st) {
    if (n <= 0 || k <= 0 || r <= 0 || r > 128 || (out && ld < k) || (geglu_half && (n != 2 * geglu_half || geglu_half % 16))) {
        set_error("dora_scale: geometry");
        return 2;
    }
    ProfScope ps("dora_scale", 2.0 * n * (double)k * r, (double)n * k * (4.0 + sizeof(T)), st);
    hipLaunchKernelGGL(dora_scale_kernel<T>, dim3((unsigned)n), dim3(256), 0, st, W, A, B, mag, s, g, reinterpret_cast<T*>(out), ld, row_off, n, k, r,
                       geglu_half, merged);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template int launch_dora_scale<float>(const float*, const float*, const float*, const float*, float, float*, void*, int, int, int, int, int, int, int,
                                      hipStream_t);
template int launch_dora_scale<bf16>(const float*, const float*, const float*, const float*, float, float*, void*, int, int, int, int, int, int, int,
                                     hipStream_t);

// ---- dora_pack_b -------------------------------------------------------------------------------------------------------------------
// dst[(row_off + dst(j)) * ld + col_off + q] = g[row_off + dst(j)] * s * B[j][q]   (launch_pack_rows with a per-row factor)
template <typename T>
__global__ void dora_pack_b_kernel(const float* __restrict__ B, const float* __restrict__ g, float s, T* __restrict__ dst, int ld, int row_off,
                                   int col_off, int n, int r, int half) {
    const long long total = (long long)n * r;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / r), q = (int)(i - (long long)j * r);
        const int dr = row_off + geglu_packed_row_or_id(j, half);
        dst[(size_t)dr * ld + col_off + q] = from_f32<T>(g[dr] * (s * B[i]));
    }
}
template <typename T>
int launch_dora_pack_b(const float* B, const float* g, float s, void* dst, int ld, int row_off, int col_off, int n, int r, int geglu_half,
                       hipStream_t st) {
    long long blocks = ((long long)n * r + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(dora_pack_b_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, B, g, s, reinterpret_cast<T*>(dst), ld, row_off, col_off, n, r,
                       geglu_half);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template int launch_dora_pack_b<float>(const float*, const float*, float, void*, int, int, int, int, int, int, hipStream_t);
template int launch_dora_pack_b<bf16>(const float*, const float*, float, void*, int, int, int, int, int, int, hipStream_t);

// ---- the refresh of a trained module's B views (Model::lora_refresh) ------------------------------------------------------------------
// v = g[row] s B[j][q], row = row0 + dst(j):  loraB[row][q] = v (f32 bank, rank <= 16) or w[row][wcol + q] = v (the sB columns of [W | sB]),
// and loraBT[bt_row0 + q][row] = v
template <typename T>
__global__ void dora_refresh_b_kernel(const float* __restrict__ B, const float* __restrict__ g, float s, float* loraB, T* w, int ldw, int wcol,
                                      T* loraBT, int ntot, int bt_row0, int row0, int n, int r, int half) {
    const long long total = (long long)n * r;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / r), q = (int)(i - (long long)j * r);
        const int row = row0 + geglu_packed_row_or_id(j, half);
        const float v = g[row] * (s * B[i]);
        if (loraB) loraB[(size_t)row * r + q] = v;
        if (w) w[(size_t)row * ldw + wcol + q] = from_f32<T>(v);
        loraBT[(size_t)(bt_row0 + q) * ntot + row] = from_f32<T>(v);
    }
}
template <typename T>
int launch_dora_refresh_b(const float* B, const float* g, float s, float* loraB, void* w, int ldw, int wcol, void* loraBT, int ntot, int bt_row0,
                          int row0, int n, int r, int geglu_half, hipStream_t st) {
    long long blocks = ((long long)n * r + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(dora_refresh_b_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, B, g, s, loraB, reinterpret_cast<T*>(w), ldw, wcol,
                       reinterpret_cast<T*>(loraBT), ntot, bt_row0, row0, n, r, geglu_half);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template int launch_dora_refresh_b<float>(const float*, const float*, float, float*, void*, int, int, void*, int, int, int, int, int, int, hipStream_t);
template int launch_dora_refresh_b<bf16>(const float*, const float*, float, float*, void*, int, int, void*, int, int, int, int, int, int, hipStream_t);

// out[j][q] += g[row0 + dst(j)] * tmp[j][q]: this step's dB (reduced into tmp, raw row order) enters the gradient scaled per row
__global__ void dora_rowscale_add_kernel(const float* __restrict__ tmp, const float* __restrict__ g, float* out, int row0, int n, int r, int half) {
    const long long total = (long long)n * r;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int j = (int)(i / r);
        out[i] += g[row0 + geglu_packed_row_or_id(j, half)] * tmp[i];
    }
}
int launch_dora_rowscale_add(const float* tmp, const float* g, float* out, int row0, int n, int r, int geglu_half, hipStream_t st) {
    long long blocks = ((long long)n * r + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(dora_rowscale_add_kernel, dim3((unsigned)blocks), dim3(256), 0, st, tmp, g, out, row0, n, r, geglu_half);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- dora_mag_grad -----------------------------------------------------------------------------------------------------------------
// gm[c] += ( sum_m P[m][src(c)] (Y[m][src(c)] - R[m][src(c)]) - bias[src(c)] sum_m P[m][src(c)] ) / mag[c]
// A workgroup owns a strip of 16 lanes x VE columns and a slab of rows, 16 row lanes deep; every lane reads 16 bytes of P, Y (and R) per row.
// The 16 row lanes fold through LDS in lane order, the slab partials (two sums per column) go to scratch with plain stores, and the reduce
// kernel adds them in slab order.
struct DoraGeom { int gx, gy, rpb, Cp; };
static DoraGeom dora_mag_grad_geom(int M, int C, int VE) {
    DoraGeom d;
    const int strip = 16 * VE;
    d.gx = (C + strip - 1) / strip;
    d.Cp = d.gx * strip;
    d.rpb = 256;
    d.gy = (M + d.rpb - 1) / d.rpb;
    if (d.gy > 64) {
        d.rpb = ((M + 63) / 64 + 15) / 16 * 16;
        d.gy = (M + d.rpb - 1) / d.rpb;
    }
    return d;
}
size_t dora_mag_grad_scratch_bytes(int M, int C, int elem_size) {
    const DoraGeom d = dora_mag_grad_geom(M, C, 16 / elem_size);
    return (size_t)d.gy * 2 * d.Cp * sizeof(float);
}

template <typename T>
__global__ __launch_bounds__(256) void dora_mag_grad_kernel(const T* __restrict__ P, int ldp, const T* __restrict__ Y, int ldy, const T* __restrict__ R,
                                                            int ldr, int M, int C, int rpb, int Cp, float* __restrict__ scratch) {
    constexpr int VE = DVec<T>::N;
    typedef typename DVec<T>::type vec_t;
    __shared__ float red[16][16 * VE * 2 + 1];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c0 = (blockIdx.x * 16 + cl) * VE;
    const int m_beg = blockIdx.y * rpb, m_end = min(M, m_beg + rpb);
    float apy[VE], ap[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) apy[e] = ap[e] = 0.f;
    if (c0 < C) {  // C is a multiple of VE: a live lane's vector lies inside the row
        for (int m = m_beg + rl; m < m_end; m += 16) {
            const vec_t pv = *reinterpret_cast<const vec_t*>(P + (size_t)m * ldp + c0);
            const vec_t yv = *reinterpret_cast<const vec_t*>(Y + (size_t)m * ldy + c0);
            if (R) {
                const vec_t rv = *reinterpret_cast<const vec_t*>(R + (size_t)m * ldr + c0);
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float p = to_f32(pv[e]);
                    apy[e] = fmaf(p, to_f32(yv[e]) - to_f32(rv[e]), apy[e]);
                    ap[e] += p;
                }
            } else {
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const float p = to_f32(pv[e]);
                    apy[e] = fmaf(p, to_f32(yv[e]), apy[e]);
                    ap[e] += p;
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        red[rl][(cl * VE + e) * 2] = apy[e];
        red[rl][(cl * VE + e) * 2 + 1] = ap[e];
    }
    __syncthreads();
    // 16 * VE * 2 sums per block, each over the 16 row lanes in lane order
    for (int i = threadIdx.x; i < 16 * VE * 2; i += 256) {
        float acc = 0.f;
#pragma unroll
        for (int l = 0; l < 16; ++l) acc += red[l][i];
        const int col = blockIdx.x * 16 * VE + (i >> 1);  // < Cp
        scratch[((size_t)blockIdx.y * 2 + (i & 1)) * Cp + col] = acc;
    }
}
__global__ void dora_mag_grad_reduce_kernel(const float* __restrict__ scratch, int gy, int Cp, const float* __restrict__ bias,
                                            const float* __restrict__ mag, float* __restrict__ gm, int C, int half) {
    const int c = blockIdx.x * 256 + threadIdx.x;  // raw row of the magnitude
    if (c >= C) return;
    const int sc = geglu_packed_row_or_id(c, half);
    float spy = 0.f, sp = 0.f;
    for (int y = 0; y < gy; ++y) {
        spy += scratch[((size_t)y * 2) * Cp + sc];
        sp += scratch[((size_t)y * 2 + 1) * Cp + sc];
    }
    const float b = bias ? bias[sc] : 0.f;
    gm[c] += (spy - b * sp) / mag[c];
}

template <typename T>
int launch_dora_mag_grad(const void* P, int ldp, const void* Y, int ldy, const void* R, int ldr, const float* bias, const float* mag, float* gm,
                         int M, int C, int geglu_half, float* scratch, hipStream_t st) {
    constexpr int VE = DVec<T>::N;
    if (M <= 0 || C <= 0 || C % VE || ldp < C || ldy < C || (R && ldr < C) || ldp % VE || ldy % VE || (R && ldr % VE) ||
        (geglu_half && (C != 2 * geglu_half || geglu_half % 16))) {
        set_error("dora_mag_grad: geometry");
        return 2;
    }
    const DoraGeom d = dora_mag_grad_geom(M, C, VE);
    ProfScope ps("dora_mag_grad", 4.0 * M * (double)C, (double)M * C * sizeof(T) * (R ? 3.0 : 2.0), st);
    hipLaunchKernelGGL(dora_mag_grad_kernel<T>, dim3(d.gx, d.gy), dim3(256), 0, st, reinterpret_cast<const T*>(P), ldp, reinterpret_cast<const T*>(Y),
                       ldy, reinterpret_cast<const T*>(R), ldr, M, C, d.rpb, d.Cp, scratch);
    MRISR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(dora_mag_grad_reduce_kernel, dim3((C + 255) / 256), dim3(256), 0, st, scratch, d.gy, d.Cp, bias, mag, gm, C, geglu_half);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template int launch_dora_mag_grad<float>(const void*, int, const void*, int, const void*, int, const float*, const float*, float*, int, int, int, float*,
                                         hipStream_t);
template int launch_dora_mag_grad<bf16>(const void*, int, const void*, int, const void*, int, const float*, const float*, float*, int, int, int, float*,
                                        hipStream_t);

}  // namespace mrisr
