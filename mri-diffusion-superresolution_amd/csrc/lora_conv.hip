// LoRA on a 3x3 conv (peft lora.Conv2d, stride 1, pad 1):  y = conv(x, W) + b + s * B (conv3x3(x, A)),  A [r][cin][3][3], B [cout][r][1][1].
// The rank-r up-projection s B z rides in the conv GEMM's epilogue (GemmArgs::lora_z); this file holds what the linears' adapters have no
// counterpart for: the 3x3 down-projection z = conv3x3(x, A) onto r <= 16 channels, its transposed conv in the backward, and the packer
// that turns the flat f32 adapter (PyTorch layouts) into the device views the kernels read.
//   Av   [R][ky][kx][cin]  compute dtype     forward down-projection (and the f32 dgrad, read with the taps flipped)
//   bank [cin][KP]         bf16              dgrad: bank[ci][t * R + q] = A[q][8 - t][ci], KP = 9 R rounded up to 32, pads zero
//   sB   [cout][r]         f32  = s * B      the conv's epilogue
//   sBT  [R][cout]         compute dtype     = s * B^T: dz = dY (s B) through launch_lora_down
#include <algorithm>

#include "common.h"
#include "prof.h"

namespace mrisr {

__device__ __forceinline__ float lc_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

int conv_lora_kpad(int R) { return (9 * R + 31) / 32 * 32; }

// ------------------------------------------------------------------------------------------------
// z[m][q] = sum_{tap, ci} x[pix(m) + tap][ci] * A[q][tap][ci]
// ------------------------------------------------------------------------------------------------
// any dtype / channel count: one wave per pixel, lanes stride over 16-byte chunks of the channels of each in-image tap
template <typename T, int RMAX>
__global__ __launch_bounds__(256) void conv_lora_down_kernel(const T* __restrict__ x, const T* __restrict__ A, float* __restrict__ z, int H, int W,
                                                             int cin, int R, int M) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int ox = m % W, oy = (m / W) % H, b = m / (W * H);
    float acc[RMAX];
#pragma unroll
    for (int q = 0; q < RMAX; ++q) acc[q] = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int iy = oy + ky - 1, ix = ox + kx - 1;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;  // (one pixel per wave: uniform)
        const T* xp = x + (((size_t)b * H + iy) * W + ix) * cin;
        const T* ap = A + (size_t)tap * cin;
        for (int k = lane * VE; k < cin; k += 64 * VE) {
            float xv[VE];
            if constexpr (sizeof(T) == 2) {
                const bf16x8 t = *reinterpret_cast<const bf16x8*>(xp + k);
#pragma unroll
                for (int e = 0; e < VE; ++e) xv[e] = (float)t[e];
            } else {
                const f32x4 t = *reinterpret_cast<const f32x4*>(xp + k);
#pragma unroll
                for (int e = 0; e < VE; ++e) xv[e] = t[e];
            }
#pragma unroll
            for (int q = 0; q < RMAX; ++q) {
                if (q < R) {
                    if constexpr (sizeof(T) == 2) {
                        const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + (size_t)q * 9 * cin + k);
#pragma unroll
                        for (int e = 0; e < VE; ++e) acc[q] += xv[e] * (float)a[e];
                    } else {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(ap + (size_t)q * 9 * cin + k);
#pragma unroll
                        for (int e = 0; e < VE; ++e) acc[q] += xv[e] * a[e];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RMAX; ++q) {
        if (q < R) {
            const float s = lc_wsum(acc[q]);
            if (lane == 0) z[(size_t)m * R + q] = s;
        }
    }
}

// bf16 on the matrix cores, in the form of lora_down_mfma_kernel: a wave owns 16 consecutive pixels (they may straddle image rows and
// images: every lane decodes its own pixel); per tap and 32-channel step it loads one row fragment - zeros where the tap leaves the image -
// and one adapter fragment straight into operand layout.  The 9 cin / 32 steps are cut into gridDim.y * NW contiguous parts:
//   NW = 1: the four waves of a workgroup take four pixel groups (pixel-parallel)
//   NW = 4: the four waves take one pixel group and a quarter of its steps each, summed through LDS in wave order
// and with gridDim.y > 1 every workgroup writes its sum to slab blockIdx.y of `out` ([gridDim.y][M][R]) for conv_lora_down_reduce_kernel.
template <int NW>
__global__ __launch_bounds__(256) void conv_lora_down_mfma_kernel(const bf16* __restrict__ x, const bf16* __restrict__ A, float* __restrict__ out,
                                                                  int H, int W, int cin, int R, int M) {
    __shared__ float red[NW == 1 ? 4 : 3 * 256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int m0 = (NW == 1 ? blockIdx.x * 4 + wv : blockIdx.x) * 16;
    if (m0 >= M) return;  // (NW = 4: the whole workgroup)
    const int cs = cin / 32, S = 9 * cs;
    const int parts = gridDim.y * NW, part = blockIdx.y * NW + (NW == 1 ? 0 : wv);
    const int lo = (int)((long long)S * part / parts), hi = (int)((long long)S * (part + 1) / parts);
    const int m = min(m0 + fr, M - 1);
    const int ox = m % W, oy = (m / W) % H, b = m / (W * H);
    const bf16* arow = A + (size_t)min(fr, R - 1) * 9 * cin + fg * 8;
    const bf16x8 zero8 = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tap = lo / cs; tap < 9 && tap * cs < hi; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int iy = oy + ky - 1, ix = ox + kx - 1;
        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
        // (a lane whose tap is outside reads its own pixel instead - a valid address - and drops the value)
        const bf16* xp = x + (((size_t)b * H + (in ? iy : oy)) * W + (in ? ix : ox)) * cin + fg * 8;
        const bf16* ap = arow + (size_t)tap * cin;
        const int c_lo = max(lo, tap * cs) - tap * cs, c_hi = min(hi, (tap + 1) * cs) - tap * cs;
        for (int c = c_lo; c < c_hi; ++c) {
            bf16x8 xf = *reinterpret_cast<const bf16x8*>(xp + c * 32);
            if (!in) xf = zero8;
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(ap + c * 32);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, af, acc, 0, 0, 0);  // D[pixel = 4fg+r][q = fr]
        }
    }
    if constexpr (NW > 1) {
        if (wv > 0) *reinterpret_cast<f32x4*>(red + (wv - 1) * 256 + lane * 4) = acc;
        __syncthreads();
        if (wv > 0) return;
#pragma unroll
        for (int w = 0; w < NW - 1; ++w) acc += *reinterpret_cast<const f32x4*>(red + w * 256 + lane * 4);
    }
    if (fr >= R) return;
    float* o = out + (size_t)blockIdx.y * M * R;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mm = m0 + fg * 4 + r;
        if (mm < M) o[(size_t)mm * R + fr] = acc[r];
    }
}
__global__ __launch_bounds__(256) void conv_lora_down_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ z, int n, int ks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = slabs[i];
    for (int k = 1; k < ks; ++k) s += slabs[(size_t)k * n + i];
    z[i] = s;
}

// Which form serves a shape (measured at the four level geometries of B = 32): the four waves of a workgroup always
// split K - at M = 32,768 that form ties the pixel-parallel one at cin = 320 and beats it by 5 - 7 % at cin = 640 / 960, below that the
// pixel-parallel grid leaves CUs idle (2.3x - 12x slower) - and the workgroups split it further, in powers of two up to 8, until there are
// two workgroups per CU, as long as every wave keeps at least 8 MFMA steps.  The pixel-parallel form stays reachable through `route`.
static void conv_lora_down_plan(int M, int cin, int route, int* nw, int* ks) {
    const int groups = (M + 15) / 16, steps = 9 * (cin / 32);
    if (route > 0) {  // forced (the op entry point's `route` = 100 * waves-per-group + K slabs: measurements and tests)
        *nw = route / 100 == 1 ? 1 : 4;
        *ks = std::max(1, std::min(route % 100, 16));
    } else {
        *nw = 4; *ks = 1;
        while (groups * *ks < 512 && *ks < 8 && steps / (4 * *ks * 2) >= 8) *ks *= 2;
    }
    while (*ks > 1 && steps / (*nw * *ks) < 1) *ks /= 2;
}
size_t conv_lora_down_scratch_bytes(int M, int cin, int R, int elem_size, int route) {
    if (elem_size != 2 || cin % 32 != 0) return 0;
    int nw, ks;
    conv_lora_down_plan(M, cin, route, &nw, &ks);
    return ks > 1 ? (size_t)ks * M * R * sizeof(float) : 0;
}

template <typename T>
int launch_conv_lora_down(const void* x, const void* A, float* z, int B, int H, int W, int cin, int R, float* scratch, hipStream_t st, int route) {
    const long long Ml = (long long)B * H * W;
    MRISR_REQUIRE(R >= 1 && R <= 16 && cin % (16 / (int)sizeof(T)) == 0 && Ml > 0 && Ml * std::max(cin, 16) < (1ll << 31), "conv_lora_down: rank <= 16, channel alignment, size");
    const int M = (int)Ml;
    ProfScope ps("conv_lora_down", 2.0 * M * (double)R * 9 * cin, (double)M * cin * sizeof(T), st);
    if (sizeof(T) == 2 && cin % 32 == 0) {
        int nw, ks;
        conv_lora_down_plan(M, cin, route, &nw, &ks);
        MRISR_REQUIRE(ks == 1 || scratch, "conv_lora_down: K-slab scratch");
        float* out = ks > 1 ? scratch : z;
        const bf16* xp = reinterpret_cast<const bf16*>(x);
        const bf16* ap = reinterpret_cast<const bf16*>(A);
        const int groups = (M + 15) / 16;
        if (nw == 1) hipLaunchKernelGGL((conv_lora_down_mfma_kernel<1>), dim3((groups + 3) / 4, ks), dim3(256), 0, st, xp, ap, out, H, W, cin, R, M);
        else hipLaunchKernelGGL((conv_lora_down_mfma_kernel<4>), dim3(groups, ks), dim3(256), 0, st, xp, ap, out, H, W, cin, R, M);
        if (ks > 1) hipLaunchKernelGGL(conv_lora_down_reduce_kernel, dim3((M * R + 255) / 256), dim3(256), 0, st, scratch, z, M * R, ks);
        MRISR_CHECK_HIP(hipGetLastError());
        return 0;
    }
    const dim3 grid((M + 3) / 4);
    const T* xp = reinterpret_cast<const T*>(x);
    const T* ap = reinterpret_cast<const T*>(A);
    if (R <= 4) hipLaunchKernelGGL((conv_lora_down_kernel<T, 4>), grid, dim3(256), 0, st, xp, ap, z, H, W, cin, R, M);
    else if (R <= 8) hipLaunchKernelGGL((conv_lora_down_kernel<T, 8>), grid, dim3(256), 0, st, xp, ap, z, H, W, cin, R, M);
    else hipLaunchKernelGGL((conv_lora_down_kernel<T, 16>), grid, dim3(256), 0, st, xp, ap, z, H, W, cin, R, M);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// dx[m][ci] (+)= sum_{tap, q} dz[pix(m) - tap][q] * A[q][tap][ci]   (the transposed conv of the r-channel gradient)
// ------------------------------------------------------------------------------------------------
// any dtype: a thread produces 4 consecutive channels of one pixel; with t the offset of the dz pixel it reads, the filter tap is 8 - t
template <typename T>
__global__ __launch_bounds__(256) void conv_lora_dgrad_kernel(const float* __restrict__ dz, const T* __restrict__ A, T* __restrict__ dx, int H, int W,
                                                              int cin, int R, int M, int accumulate) {
    const int C4 = cin / 4;
    const long long total = (long long)M * C4;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C4) * 4, m = (int)(i / C4);
        const int ox = m % W, oy = (m / W) % H, b = m / (W * H);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < 9; ++t) {
            const int ty = t / 3, tx = t - ty * 3;
            const int iy = oy + ty - 1, ix = ox + tx - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const float* dp = dz + (((size_t)b * H + iy) * W + ix) * R;
            const T* ap = A + (size_t)(8 - t) * cin + c;
            for (int q = 0; q < R; ++q) {
                const float d = dp[q];
                const T* aq = ap + (size_t)q * 9 * cin;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += d * to_f32(aq[e]);
            }
        }
        T* o = dx + (size_t)m * cin + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(acc[e] + (accumulate ? to_f32(o[e]) : 0.f));
    }
}

// bf16 on the matrix cores, the sibling of conv_in_mfma_kernel with the roles of the channel counts exchanged: R input channels (K = 9 R padded
// to KP = 64 / 96 / 128 / 160), cin output channels.  A workgroup stages the bank rows of its channel chunk (blockIdx.y) in LDS once and walks
// pixel groups of 16; a wave gathers the 3x3xR neighbourhood of its pixels from dz (f32, rounded to bf16 here) straight into the column
// fragments, then runs chunk / 16 x KP / 32 MFMAs.  D[channel = 4fg+r][pixel = fr]: a lane ends with 4 consecutive channels of one pixel and
// writes (or adds into) them as one 8-byte piece.
template <int R>
__global__ __launch_bounds__(256) void conv_lora_dgrad_mfma_kernel(const float* __restrict__ dz, const bf16* __restrict__ bank, bf16* __restrict__ dx,
                                                                   int H, int W, int cin, int M, int CH, int accumulate) {
    constexpr int NS = (9 * R + 31) / 32, KP = NS * 32, LP = KP + 8;
    extern __shared__ __attribute__((aligned(16))) char sm_raw[];
    bf16* bl = reinterpret_cast<bf16*>(sm_raw);  // [nch][LP]
    const int c0 = blockIdx.y * CH, nch = min(CH, cin - c0);
    for (int i = threadIdx.x; i < nch * (KP / 8); i += 256) {
        const int n = i / (KP / 8), j = i - n * (KP / 8);
        *reinterpret_cast<uint4*>(bl + (size_t)n * LP + j * 8) = *reinterpret_cast<const uint4*>(bank + (size_t)(c0 + n) * KP + j * 8);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, fr = lane & 15, fg = lane >> 4;
    const int ngroups = (M + 15) / 16;
    for (int pg = blockIdx.x * 4 + (threadIdx.x >> 6); pg < ngroups; pg += gridDim.x * 4) {
        const int m = pg * 16 + fr;
        bf16x8 af[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) af[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (m < M) {
            const int ox = m % W, oy = (m / W) % H, b = m / (W * H);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k0 = s * 32 + fg * 8 + h * 4;  // 4 consecutive k share a tap (R is a multiple of 4)
                    const int t = k0 / R, q0 = k0 - t * R;
                    const int ty = t / 3, tx = t - ty * 3;
                    const int iy = oy + ty - 1, ix = ox + tx - 1;
                    if (t < 9 && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(dz + (((size_t)b * H + iy) * W + ix) * R + q0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) af[s][h * 4 + e] = (bf16)v[e];
                    }
                }
            }
        }
        for (int i = 0; i < nch / 16; ++i) {
            const bf16* wr = bl + (size_t)(i * 16 + fr) * LP + fg * 8;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NS; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(wr + s * 32), af[s], acc, 0, 0, 0);
            if (m < M) {
                bf16* o = dx + (size_t)m * cin + c0 + i * 16 + fg * 4;
                bf16x4 ov;
                if (accumulate) {
                    const bf16x4 p = *reinterpret_cast<const bf16x4*>(o);
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = (bf16)(acc[r] + (float)p[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = (bf16)acc[r];
                }
                *reinterpret_cast<bf16x4*>(o) = ov;
            }
        }
    }
}

// A: the Av view [R][9][cin] (the direct kernel); bank: [cin][KP] bf16 (the matrix-core kernel: bf16, R in {4, 8, 12, 16}, cin % 16 == 0)
template <typename T>
int launch_conv_lora_dgrad(const float* dz, const void* A, const void* bank, void* dx, int B, int H, int W, int cin, int R, int accumulate,
                           hipStream_t st) {
    const long long Ml = (long long)B * H * W;
    MRISR_REQUIRE(R >= 1 && R <= 16 && cin % 4 == 0 && Ml > 0 && Ml * cin < (1ll << 31), "conv_lora_dgrad: rank <= 16, channel alignment, size");
    const int M = (int)Ml;
    ProfScope ps("conv_lora_dgrad", 2.0 * M * (double)R * 9 * cin, (double)M * cin * sizeof(T) * (accumulate ? 2 : 1), st);
    if (sizeof(T) == 2 && bank && R % 4 == 0 && cin % 16 == 0) {
        const int CH = R == 4 ? 256 : 128, nchunks = (cin + CH - 1) / CH;  // <= 42 KB of LDS
        const int KP = conv_lora_kpad(R);
        const size_t smem = (size_t)std::min(CH, cin) * (KP + 8) * 2;
        const int groups = (M + 15) / 16;
        const int gx = std::max(1, std::min((groups + 3) / 4, 1024 / nchunks));
        const dim3 grid(gx, nchunks);
        const bf16* bp = reinterpret_cast<const bf16*>(bank);
        bf16* op = reinterpret_cast<bf16*>(dx);
        switch (R) {
            case 4: hipLaunchKernelGGL((conv_lora_dgrad_mfma_kernel<4>), grid, dim3(256), smem, st, dz, bp, op, H, W, cin, M, CH, accumulate); break;
            case 8: hipLaunchKernelGGL((conv_lora_dgrad_mfma_kernel<8>), grid, dim3(256), smem, st, dz, bp, op, H, W, cin, M, CH, accumulate); break;
            case 12: hipLaunchKernelGGL((conv_lora_dgrad_mfma_kernel<12>), grid, dim3(256), smem, st, dz, bp, op, H, W, cin, M, CH, accumulate); break;
            default: hipLaunchKernelGGL((conv_lora_dgrad_mfma_kernel<16>), grid, dim3(256), smem, st, dz, bp, op, H, W, cin, M, CH, accumulate); break;
        }
        MRISR_CHECK_HIP(hipGetLastError());
        return 0;
    }
    MRISR_REQUIRE(A, "conv_lora_dgrad: adapter view");
    long long blocks = ((long long)M * (cin / 4) + 255) / 256;
    if (blocks > 65535 * 4) blocks = 65535 * 4;
    hipLaunchKernelGGL(conv_lora_dgrad_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, dz, reinterpret_cast<const T*>(A), reinterpret_cast<T*>(dx), H, W,
                       cin, R, M, accumulate);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// pack / refresh: flat f32 adapter (A [r][cin][3][3], B [cout][r]) -> the four device views
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void conv_lora_pack_kernel(const float* __restrict__ A, const float* __restrict__ Bm, float s, T* Av, bf16* bank, float* sB, T* sBT, int cin,
                                      int cout, int r, int KP) {
    const long long na = (long long)r * cin * 9, nb = (long long)cout * r;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256) {
        if (i < na) {
            const int q = (int)(i / (cin * 9)), rem = (int)(i - (long long)q * cin * 9);
            const int ci = rem / 9, tap = rem - ci * 9;
            const float v = A[i];
            Av[((size_t)q * 9 + tap) * cin + ci] = from_f32<T>(v);
            if (bank) bank[(size_t)ci * KP + (8 - tap) * r + q] = (bf16)v;
        } else {
            const long long j = i - na;
            const int c = (int)(j / r), q = (int)(j - (long long)c * r);
            const float v = s * Bm[j];
            if (sB) sB[j] = v;
            if (sBT) sBT[(size_t)q * cout + c] = from_f32<T>(v);
        }
    }
}
template <typename T>
int launch_conv_lora_pack(const float* A, const float* Bm, float s, void* Av, void* bank, float* sB, void* sBT, int cin, int cout, int r, hipStream_t st) {
    MRISR_REQUIRE(A && Bm && Av && r >= 1 && r <= 16, "conv adapter pack: operands");
    const long long total = (long long)r * cin * 9 + (long long)cout * r;
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(conv_lora_pack_kernel<T>, dim3(blocks), dim3(256), 0, st, A, Bm, s, reinterpret_cast<T*>(Av), reinterpret_cast<bf16*>(bank), sB,
                       reinterpret_cast<T*>(sBT), cin, cout, r, conv_lora_kpad(r));
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

// f32 rows -> compute dtype (dz as the r-column dY of the adapter's conv_wgrad_run)
template <typename T>
__global__ void cast_rows_kernel(const float* __restrict__ src, T* __restrict__ dst, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = from_f32<T>(src[i]);
}
template <typename T>
int launch_cast_rows(const float* src, void* dst, long long n, hipStream_t st) {
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(cast_rows_kernel<T>, dim3(blocks), dim3(256), 0, st, src, reinterpret_cast<T*>(dst), n);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

#define LORA_CONV_INST(T)                                                                                                               \
    template int launch_conv_lora_down<T>(const void*, const void*, float*, int, int, int, int, int, float*, hipStream_t, int);         \
    template int launch_conv_lora_dgrad<T>(const float*, const void*, const void*, void*, int, int, int, int, int, int, hipStream_t);   \
    template int launch_conv_lora_pack<T>(const float*, const float*, float, void*, void*, float*, void*, int, int, int, hipStream_t);  \
    template int launch_cast_rows<T>(const float*, void*, long long, hipStream_t);
LORA_CONV_INST(float)
LORA_CONV_INST(bf16)

}  // namespace mrisr
