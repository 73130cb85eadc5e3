// FreeU (Si et al. 2023; diffusers' apply_freeu / fourier_filter): one launch per decoder stage on the two NHWC
// operands of the stage's resnet, before its (implicit) concat.
//
//   backbone   hidden[b][p][c] *= bscale                  for c < Ch / 2; the other channels are copied (out of place) or left alone
//   skip       fourier_filter(skip, threshold = 1, scale = s) per (sample, channel) plane of H x W pixels
//
// The filter multiplies by s the 2 x 2 block [H/2-1 : H/2+1, W/2-1 : W/2+1] of the shifted spectrum: the frequencies ky in {0, H-1},
// kx in {0, W-1} as distinct residues (H == 1 or W == 1 leaves one on that axis).  With a = 2 pi y / H and b = 2 pi x / W the up to four
// forward coefficients are seven real sums over the plane,
//   S0 = sum x      (Syc, Sys) = sum x (cos a, sin a)      (Sxc, Sxs) = sum x (cos b, sin b)      (Sr, Si) = sum x (cos(a+b), sin(a+b))
// and the real part of the masked inverse transform is
//   y = x + (s - 1) / (H W) (S0 + [H>1] (Syc cos a + Sys sin a) + [W>1] (Sxc cos b + Sxs sin b) + [H>1][W>1] (Sr cos(a+b) + Si sin(a+b)))
// No FFT: the planes hold at most a few hundred pixels.
//
// A workgroup of FU_CV x FU_PS threads owns FU_CV 16-byte channel pieces of one sample: lanes run along C (a 32-lane half reads 512
// contiguous bytes of one pixel), the FU_PS slices stride over the pixels.  Pass 1 accumulates the sums in f32 registers, the slices'
// partials meet in LDS and every thread adds them in the same fixed order (no atomics: the bits repeat from launch to launch); pass 2 reads
// the plane again and writes the filtered values, rounded once.  Every pixel is read and written by the same thread, and the barrier
// between the passes orders all reads of pass 1 before any write, so skip_out may be skip.  The twiddles come from sincospif, once per
// workgroup, and live in LDS.  The workgroups after the skip's scale the backbone half in 16-byte pieces, one element read and written
// by one lane (hidden_out may be hidden).
//
// The two scalars come by value, or - a run with a per-step schedule - from row *step of the sampler's schedule table
// [n_steps][8]: columns col_b and col_s, read with ordinary loads by every thread (one cache line, uniform over the launch).  The row
// (b, s) = (1, 1) changes no bit: v * 1 is exact and (s - 1) / (H W) is 0, so the correction term is 0 * t.
#include <algorithm>
#include <cmath>

#include "api.h"
#include "prof.h"
#include "runtime.h"

namespace mrisr {

constexpr int FU_CV = 32;                 // 16-byte channel pieces per workgroup
constexpr int FU_PS = 4;                  // pixel slices per workgroup
constexpr int FU_THREADS = FU_CV * FU_PS;
constexpr int FU_MAX_HW = 1024;           // largest H and W (the twiddle tables: 2 floats per row / column of LDS)

template <typename T>
__global__ __launch_bounds__(FU_THREADS) void freeu_kernel(const T* hid, const T* skip, T* hid_out, T* skip_out, int H, int W, int Ch, int Cs, float bscale, float s,
                                                           int skip_blocks, int cs_chunks, int hid_blocks, long long hid_vecs, int hid_cw,
                                                           const float* sched, const int* step, int col_b, int col_s) {
    constexpr int VE = 16 / (int)sizeof(T);
    union Vec { uint4 q; T e[VE]; };
    extern __shared__ float fu_lds[];
    if (sched) {
        const float* row = sched + 8 * (size_t)*step;
        bscale = row[col_b];
        s = row[col_s];
    }
    if ((int)blockIdx.x >= skip_blocks) {
        // ---- backbone: hid_cw channels of every pixel row (Ch / 2 in place, Ch out of place), the first Ch / 2 scaled
        const int vpr = hid_cw / VE, half = Ch / 2;
        for (long long v = (long long)(blockIdx.x - skip_blocks) * FU_THREADS + threadIdx.x; v < hid_vecs; v += (long long)hid_blocks * FU_THREADS) {
            const long long row = v / vpr;
            const int c = (int)(v - row * vpr) * VE;
            Vec u;
            u.q = *reinterpret_cast<const uint4*>(hid + row * Ch + c);
            if (c < half) {
#pragma unroll
                for (int k = 0; k < VE; ++k) u.e[k] = from_f32<T>(to_f32(u.e[k]) * bscale);
            }
            *reinterpret_cast<uint4*>(hid_out + row * Ch + c) = u.q;
        }
        return;
    }
    // ---- skip
    float* tw = fu_lds;                   // [H] (cos a, sin a), then [W] (cos b, sin b)
    float* red = fu_lds + 2 * (H + W);    // [FU_PS][7][FU_CV * VE]
    for (int i = threadIdx.x; i < H + W; i += FU_THREADS) {
        float sn, cs;
        if (i < H) sincospif(2.0f * (float)i / (float)H, &sn, &cs);
        else sincospif(2.0f * (float)(i - H) / (float)W, &sn, &cs);
        tw[2 * i] = cs;
        tw[2 * i + 1] = sn;
    }
    __syncthreads();
    const int cv = threadIdx.x % FU_CV, ps = threadIdx.x / FU_CV;
    const int b = blockIdx.x / cs_chunks, chunk = blockIdx.x % cs_chunks;
    const int c0 = (chunk * FU_CV + cv) * VE;
    const bool live = c0 < Cs;
    const int HW = H * W;
    const float fy = H > 1 ? 1.f : 0.f, fx = W > 1 ? 1.f : 0.f, fxy = fy * fx;
    const T* src = skip + (size_t)b * HW * Cs + c0;
    T* dst = skip_out + (size_t)b * HW * Cs + c0;
    float acc[7][VE];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < VE; ++e) acc[k][e] = 0.f;
    if (live) {
        for (int p = ps; p < HW; p += FU_PS) {
            const int y = p / W, x = p - y * W;
            const float cy = tw[2 * y], sy = tw[2 * y + 1], cx = tw[2 * (H + x)], sx = tw[2 * (H + x) + 1];
            const float cr = cy * cx - sy * sx, ci = sy * cx + cy * sx;
            Vec u;
            u.q = *reinterpret_cast<const uint4*>(src + (size_t)p * Cs);
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const float v = to_f32(u.e[e]);
                acc[0][e] += v;
                acc[1][e] += v * cy; acc[2][e] += v * sy;
                acc[3][e] += v * cx; acc[4][e] += v * sx;
                acc[5][e] += v * cr; acc[6][e] += v * ci;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < VE; ++e) red[(ps * 7 + k) * (FU_CV * VE) + cv * VE + e] = acc[k][e];
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            float t = red[k * (FU_CV * VE) + cv * VE + e];
#pragma unroll
            for (int q = 1; q < FU_PS; ++q) t += red[(q * 7 + k) * (FU_CV * VE) + cv * VE + e];
            acc[k][e] = t;
        }
    const float g = (s - 1.0f) / (float)HW;
    for (int p = ps; p < HW; p += FU_PS) {
        const int y = p / W, x = p - y * W;
        const float cy = fy * tw[2 * y], sy = fy * tw[2 * y + 1], cx = fx * tw[2 * (H + x)], sx = fx * tw[2 * (H + x) + 1];
        const float cr = fxy * (tw[2 * y] * tw[2 * (H + x)] - tw[2 * y + 1] * tw[2 * (H + x) + 1]);
        const float ci = fxy * (tw[2 * y + 1] * tw[2 * (H + x)] + tw[2 * y] * tw[2 * (H + x) + 1]);
        Vec u;
        u.q = *reinterpret_cast<const uint4*>(src + (size_t)p * Cs);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const float t = acc[0][e] + (acc[1][e] * cy + acc[2][e] * sy) + (acc[3][e] * cx + acc[4][e] * sx) + (acc[5][e] * cr + acc[6][e] * ci);
            u.e[e] = from_f32<T>(to_f32(u.e[e]) + g * t);
        }
        *reinterpret_cast<uint4*>(dst + (size_t)p * Cs) = u.q;
    }
}

// b, s by value (sched == nullptr) or from the schedule table (sched, step, col_b, col_s)
template <typename T>
static int launch_freeu_impl(const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs, float b,
                             float s, const float* sched, const int* step, int col_b, int col_s, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    MRISR_REQUIRE(hidden && skip && hidden_out && skip_out, "freeu: null operand");
    MRISR_REQUIRE(((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(skip) | reinterpret_cast<uintptr_t>(hidden_out) |
                    reinterpret_cast<uintptr_t>(skip_out)) % 16) == 0, "freeu: operands must be 16-byte aligned");
    MRISR_REQUIRE(B >= 1 && H >= 1 && W >= 1, "freeu: B, H and W must be at least 1");
    MRISR_REQUIRE(H <= FU_MAX_HW && W <= FU_MAX_HW, "freeu: H and W at most 1024");
    MRISR_REQUIRE(Ch >= 16 && Ch % 16 == 0, "freeu: the hidden channels must be a multiple of 16");
    MRISR_REQUIRE(Cs >= 8 && Cs % 8 == 0, "freeu: the skip channels must be a multiple of 8");
    if (sched)  // the values were checked when the table was set (mrisr_sampler_set_schedule)
        MRISR_REQUIRE(step && col_b >= 3 && col_b <= 6 && col_s >= 3 && col_s <= 6, "freeu: schedule table without a step counter, or a column outside 3..6");
    else
        MRISR_REQUIRE(std::isfinite(b) && b >= 0.f && std::isfinite(s) && s >= 0.f, "freeu: b and s must be finite and >= 0");
    const int cs_chunks = (Cs / VE + FU_CV - 1) / FU_CV;
    const long long skip_blocks = (long long)B * cs_chunks;
    const int hid_cw = hidden_out == hidden ? Ch / 2 : Ch;
    const long long hid_vecs = (long long)B * H * W * (hid_cw / VE);
    const long long hid_blocks = std::min<long long>((hid_vecs + FU_THREADS * 4 - 1) / (FU_THREADS * 4), 4096);
    MRISR_REQUIRE(skip_blocks + hid_blocks < (1ll << 31), "freeu: too many workgroups for one launch");
    const size_t lds = (size_t)(2 * (H + W) + FU_PS * 7 * FU_CV * VE) * sizeof(float);
    ProfScope ps("freeu", 0.0, (double)B * H * W * (3.0 * Cs + 2.0 * hid_cw) * sizeof(T), st);
    hipLaunchKernelGGL(freeu_kernel<T>, dim3((unsigned)(skip_blocks + hid_blocks)), dim3(FU_THREADS), lds, st, static_cast<const T*>(hidden),
                       static_cast<const T*>(skip), static_cast<T*>(hidden_out), static_cast<T*>(skip_out), H, W, Ch, Cs, b, s, (int)skip_blocks,
                       cs_chunks, (int)hid_blocks, hid_vecs, hid_cw, sched, step, col_b, col_s);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template <typename T>
int launch_freeu(const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs, float b, float s,
                 hipStream_t st) {
    return launch_freeu_impl<T>(hidden, skip, hidden_out, skip_out, B, H, W, Ch, Cs, b, s, nullptr, nullptr, 0, 0, st);
}
template <typename T>
int launch_freeu_sched(const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs,
                       const float* sched, const int* step, int col_b, int col_s, hipStream_t st) {
    MRISR_REQUIRE(sched && step, "freeu: null schedule table or step counter");
    return launch_freeu_impl<T>(hidden, skip, hidden_out, skip_out, B, H, W, Ch, Cs, 1.f, 1.f, sched, step, col_b, col_s, st);
}
template int launch_freeu<float>(const void*, const void*, void*, void*, int, int, int, int, int, float, float, hipStream_t);
template int launch_freeu<bf16>(const void*, const void*, void*, void*, int, int, int, int, int, float, float, hipStream_t);
template int launch_freeu_sched<float>(const void*, const void*, void*, void*, int, int, int, int, int, const float*, const int*, int, int, hipStream_t);
template int launch_freeu_sched<bf16>(const void*, const void*, void*, void*, int, int, int, int, int, const float*, const int*, int, int, hipStream_t);

}  // namespace mrisr
