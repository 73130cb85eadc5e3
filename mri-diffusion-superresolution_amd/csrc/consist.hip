// Low-frequency consistency (ILVR): after the reverse step, the low band of the state is pulled towards the low band
// of a reference noised to the level the step produced,
//
//   x  <-  x + w phi_N( y - x ),      y = alpha ref + beta lr + sigma z,      {w, alpha, beta, sigma} = table[*step]
//
// phi_N: the mean over each N x N block, then an upsample by N back to [h, w] - bilinear (filter 0; torch's align_corners=False rule: source
// coordinate (i + 0.5) / N - 0.5, a negative one clamped to 0, the upper neighbour clamped to the last cell) or nearest (filter 1; an exact
// projection).  The table row is read behind the load of the step counter with ordinary loads, uniform over the launch: other weights replay
// the same captured graph.  A row with w == 0 returns before anything else is read: x and the staging buffer keep their bits.
//
// ONE workgroup of 256 threads per (sample, channel) plane, three passes with a barrier between them:
//   1. row sums: d = alpha ref + beta lr + sigma z - x summed over N contiguous elements, left to right  -> LDS  rs[h][w / N]
//   2. column sums: N rows of rs, top to bottom, divided by N^2                                           -> LDS  D[h / N][w / N]
//   3. every fine pixel: u interpolated from D, x = fma(w, u, x), stored to x and to every part of the [K B] staging buffer
// No atomics and one summation order whatever the path, so the bits repeat from launch to launch and between the 16-byte path (w % 4 == 0
// and 16-byte aligned operands) and the scalar one.  A workgroup touches its own plane only: the barriers order pass 1's reads of x against
// pass 3's stores.  LDS: 4 (h w / N + h w / N^2) bytes of dynamic shared memory, all accesses 32-bit.
#include <cmath>
#include <string>

#include "api.h"
#include "prof.h"
#include "runtime.h"

namespace mrisr {

__device__ __forceinline__ float consist_d(const ConsistArgs& a, float al, float be, float sg, const float* z, long long i) {
    float t = al * a.ref[i];
    if (a.lr) t = fmaf(be, a.lr[i], t);
    if (z) t = fmaf(sg, z[i], t);
    return t - a.x[i];
}
__device__ __forceinline__ float4 consist_d4(const ConsistArgs& a, float al, float be, float sg, const float* z, long long i4) {
    const float4 r = reinterpret_cast<const float4*>(a.ref)[i4], xv = reinterpret_cast<const float4*>(a.x)[i4];
    float4 t = make_float4(al * r.x, al * r.y, al * r.z, al * r.w);
    if (a.lr) {
        const float4 l = reinterpret_cast<const float4*>(a.lr)[i4];
        t = make_float4(fmaf(be, l.x, t.x), fmaf(be, l.y, t.y), fmaf(be, l.z, t.z), fmaf(be, l.w, t.w));
    }
    if (z) {
        const float4 n = reinterpret_cast<const float4*>(z)[i4];
        t = make_float4(fmaf(sg, n.x, t.x), fmaf(sg, n.y, t.y), fmaf(sg, n.z, t.z), fmaf(sg, n.w, t.w));
    }
    return make_float4(t.x - xv.x, t.y - xv.y, t.z - xv.z, t.w - xv.w);
}
// the two source cells and the weight of the upper one for fine index i = c N + r of an axis with nc cells
template <int N>
__device__ __forceinline__ void consist_tap(int i, int nc, int filter, int& i0, int& i1, float& lam) {
    const int c = i / N, r = i - c * N;
    if (filter) { i0 = i1 = c; lam = 0.f; return; }
    const int num = 2 * r + 1 - N;  // (i + 0.5) / N - 0.5 = c + num / (2 N)
    if (num >= 0) { i0 = c; lam = (float)num / (float)(2 * N); }
    else if (c == 0) { i0 = 0; lam = 0.f; }  // a negative coordinate is clamped to 0
    else { i0 = c - 1; lam = (float)(num + 2 * N) / (float)(2 * N); }
    i1 = i0 + 1 < nc ? i0 + 1 : nc - 1;
}
__device__ __forceinline__ float consist_u(const float* D, int wc, int y0, int y1, float ly, int x0, int x1, float lx) {
    const float top = (1.f - lx) * D[y0 * wc + x0] + lx * D[y0 * wc + x1];
    const float bot = (1.f - lx) * D[y1 * wc + x0] + lx * D[y1 * wc + x1];
    return (1.f - ly) * top + ly * bot;
}

template <int N, bool VEC>
__global__ __launch_bounds__(256) void consistency_kernel(ConsistArgs a) {
    extern __shared__ __attribute__((aligned(16))) char consist_smem[];
    const int s = *a.step;
    const float* row = a.table + 4 * (size_t)s;
    const float wgt = row[0];
    if (wgt == 0.f) return;  // uniform over the launch, before any barrier
    const float al = row[1], be = row[2], sg = row[3];
    const int h = a.h, w = a.w, hc = h / N, wc = w / N;
    const long long plane = (long long)h * w, n = (long long)a.B * a.C * plane;
    const long long base = (long long)blockIdx.x * plane;
    const float* z = a.noise && sg != 0.f ? a.noise + (size_t)s * n : nullptr;
    float* rs = reinterpret_cast<float*>(consist_smem);  // [h][wc]
    float* D = rs + h * wc;                               // [hc][wc]

    // pass 1: item = one run of N contiguous elements of a row; w is a multiple of N, so item j starts at base + j N
    const int items = h * wc;
    if (VEC && N == 2) {  // one 16-byte piece holds two runs
        for (int j = threadIdx.x; j < (items >> 1); j += 256) {
            const float4 d = consist_d4(a, al, be, sg, z, (base >> 2) + j);
            rs[2 * j] = d.x + d.y;
            rs[2 * j + 1] = d.z + d.w;
        }
    } else if (VEC && N % 4 == 0) {
        for (int j = threadIdx.x; j < items; j += 256) {
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {
                const float4 d = consist_d4(a, al, be, sg, z, (base >> 2) + (long long)j * (N / 4) + q);
                acc = q == 0 ? ((d.x + d.y) + d.z) + d.w : (((acc + d.x) + d.y) + d.z) + d.w;
            }
            rs[j] = acc;
        }
    } else {
        for (int j = threadIdx.x; j < items; j += 256) {
            const long long i = base + (long long)j * N;
            float acc = consist_d(a, al, be, sg, z, i);
#pragma unroll
            for (int q = 1; q < N; ++q) acc += consist_d(a, al, be, sg, z, i + q);
            rs[j] = acc;
        }
    }
    __syncthreads();
    // pass 2
    for (int j = threadIdx.x; j < hc * wc; j += 256) {
        const int cy = j / wc, cx = j - cy * wc;
        float acc = rs[(cy * N) * wc + cx];
#pragma unroll
        for (int q = 1; q < N; ++q) acc += rs[(cy * N + q) * wc + cx];
        D[j] = acc / (float)(N * N);
    }
    __syncthreads();
    // pass 3
    if (VEC) {
        const int w4 = w >> 2;
        for (int j = threadIdx.x; j < h * w4; j += 256) {
            const int y = j / w4, x4 = (j - y * w4) * 4;
            int y0, y1, x0, x1;
            float ly, lx;
            consist_tap<N>(y, hc, a.filter, y0, y1, ly);
            const long long i4 = (base >> 2) + j;
            float4 v = reinterpret_cast<const float4*>(a.x)[i4];
            consist_tap<N>(x4, wc, a.filter, x0, x1, lx);
            v.x = fmaf(wgt, consist_u(D, wc, y0, y1, ly, x0, x1, lx), v.x);
            consist_tap<N>(x4 + 1, wc, a.filter, x0, x1, lx);
            v.y = fmaf(wgt, consist_u(D, wc, y0, y1, ly, x0, x1, lx), v.y);
            consist_tap<N>(x4 + 2, wc, a.filter, x0, x1, lx);
            v.z = fmaf(wgt, consist_u(D, wc, y0, y1, ly, x0, x1, lx), v.z);
            consist_tap<N>(x4 + 3, wc, a.filter, x0, x1, lx);
            v.w = fmaf(wgt, consist_u(D, wc, y0, y1, ly, x0, x1, lx), v.w);
            reinterpret_cast<float4*>(a.x)[i4] = v;
            for (int k = 0; k < a.K; ++k) reinterpret_cast<float4*>(a.xK + k * n)[i4] = v;
        }
    } else {
        for (int j = threadIdx.x; j < h * w; j += 256) {
            const int y = j / w, xx = j - y * w;
            int y0, y1, x0, x1;
            float ly, lx;
            consist_tap<N>(y, hc, a.filter, y0, y1, ly);
            consist_tap<N>(xx, wc, a.filter, x0, x1, lx);
            const float v = fmaf(wgt, consist_u(D, wc, y0, y1, ly, x0, x1, lx), a.x[base + j]);
            a.x[base + j] = v;
            for (int k = 0; k < a.K; ++k) a.xK[k * n + base + j] = v;
        }
    }
}

// the rules of a consistency launch on numbers alone: the factor, the filter, divisibility and the LDS need of the canvas
int check_consistency_geometry(int factor, int filter, int h, int w) {
    MRISR_REQUIRE(factor >= CONSIST_MIN_FACTOR && factor <= CONSIST_MAX_FACTOR, "consistency: the factor must lie in 2 .. 8, got " + std::to_string(factor));
    MRISR_REQUIRE(filter == MRISR_CONSIST_BILINEAR || filter == MRISR_CONSIST_NEAREST, "consistency: the filter is 0 (bilinear) or 1 (nearest)");
    MRISR_REQUIRE(h > 0 && w > 0 && h % factor == 0 && w % factor == 0,
                  "consistency: the factor " + std::to_string(factor) + " must divide h and w of the latents (" + std::to_string(h) + " x " + std::to_string(w) + ")");
    MRISR_REQUIRE(consist_lds_bytes(h, w, factor) <= CONSIST_LDS_CAP,
                  "consistency: a " + std::to_string(h) + " x " + std::to_string(w) + " canvas at factor " + std::to_string(factor) + " needs " +
                      std::to_string(consist_lds_bytes(h, w, factor)) + " bytes of LDS, more than 65536: use a larger factor");
    return 0;
}
// the checks a consistency table passes before anything touches the device
int check_consistency_rows(const float* rows, int n_rows) {
    static const char* const names[4] = {"weight (w)", "alpha", "beta", "sigma"};
    for (int i = 0; i < n_rows; ++i)
        for (int c = 0; c < 4; ++c)
            MRISR_REQUIRE(std::isfinite(rows[4 * (size_t)i + c]), "consistency: row " + std::to_string(i) + ": " + names[c] + " is not finite");
    return 0;
}

template <int N>
static void launch_consistency_n(const ConsistArgs& a, bool vec, unsigned planes, size_t lds, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((consistency_kernel<N, true>), dim3(planes), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((consistency_kernel<N, false>), dim3(planes), dim3(256), lds, st, a);
}
int launch_consistency(const ConsistArgs& a, hipStream_t st) {
    MRISR_REQUIRE(a.x && a.ref && a.table && a.step, "consistency: null operand");
    MRISR_REQUIRE(a.K >= 1 && a.K <= 3, "consistency: K must lie in 1 .. 3, got " + std::to_string(a.K));
    MRISR_REQUIRE(a.K == 1 || a.xK, "consistency: more than one part needs the staging buffer");
    MRISR_REQUIRE(a.B > 0 && a.C > 0 && (long long)a.B * a.C < (1ll << 31), "consistency: empty or oversized batch");
    TRY(check_consistency_geometry(a.factor, a.filter, a.h, a.w));
    auto al = [](const void* p, int m) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(m - 1)) == 0; };
    MRISR_REQUIRE(al(a.x, 4) && al(a.xK, 4) && al(a.ref, 4) && al(a.lr, 4) && al(a.noise, 4) && al(a.table, 4) && al(a.step, 4),
                  "consistency: operands must be 4-byte aligned");
    const bool vec = a.w % 4 == 0 && al(a.x, 16) && al(a.xK, 16) && al(a.ref, 16) && al(a.lr, 16) && al(a.noise, 16);
    const unsigned planes = (unsigned)(a.B * a.C);
    const size_t lds = (size_t)consist_lds_bytes(a.h, a.w, a.factor);
    const int K = a.xK ? a.K : 0;  // an unguided run has no staging buffer: x is the only copy of the state
    ConsistArgs k = a;
    k.K = K;
    // ref, x in (twice), 1 + K stores of x; lr and the noise slab when given
    const double bytes = (4.0 * (3 + 1 + K) + (a.lr ? 4.0 : 0.0) + (a.noise ? 4.0 : 0.0)) * (double)planes * a.h * a.w;
    ProfScope ps("consistency", 0.0, bytes, st);
    switch (a.factor) {
        case 2: launch_consistency_n<2>(k, vec, planes, lds, st); break;
        case 3: launch_consistency_n<3>(k, vec, planes, lds, st); break;
        case 4: launch_consistency_n<4>(k, vec, planes, lds, st); break;
        case 5: launch_consistency_n<5>(k, vec, planes, lds, st); break;
        case 6: launch_consistency_n<6>(k, vec, planes, lds, st); break;
        case 7: launch_consistency_n<7>(k, vec, planes, lds, st); break;
        default: launch_consistency_n<8>(k, vec, planes, lds, st); break;
    }
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace mrisr
