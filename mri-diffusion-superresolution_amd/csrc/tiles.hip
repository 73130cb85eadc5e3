// Tiled sampling: the per-axis tile grid and blend window on the host, and the two kernels that stand between
// the sampler's canvas state and the forward's tile batch - gather (canvas -> tiles, a copy) and blend (tile predictions -> the canvas
// prediction the step kernels read).  f32 NCHW on both sides.  Both are memory-bound and small: one thread per 16 bytes of the side that is
// written when the geometry allows it (t_w, W and every x origin multiples of 4, 16-byte aligned bases), one thread per element otherwise.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "api.h"
#include "prof.h"
#include "runtime.h"

namespace mrisr {

// ---- the one place that computes grid and window (contract: include/mrisr.h, mrisr_tile_tables) ----
int tile_axis(int n, int t, int o, int window, std::vector<int>& origins, std::vector<float>& weights) {
    MRISR_REQUIRE(n > 0 && t > 0, "tile tables: extent and tile must be positive");
    MRISR_REQUIRE(o >= 0 && o < t, "tile tables: overlap must lie in 0 .. tile - 1");
    MRISR_REQUIRE(window == MRISR_TILE_UNIFORM || window == MRISR_TILE_GAUSSIAN, "tile tables: unknown window");
    const int te = std::min(t, n);
    origins.clear();
    if (n <= t) origins.push_back(0);
    else {
        const int s = t - o, k = (n - t + s - 1) / s + 1;
        for (int i = 0; i < k; ++i) origins.push_back(std::min(i * s, n - t));  // the last tile is pulled back to end at n
    }
    const int k = (int)origins.size();
    std::vector<double> w(te, 1.0), sum(n, 0.0);
    if (window == MRISR_TILE_GAUSSIAN)
        for (int i = 0; i < te; ++i) {
            const double u = (i - (te - 1) / 2.0) / te;
            w[i] = std::exp(-u * u / (2.0 * 0.01));
        }
    for (int q = 0; q < k; ++q)
        for (int i = 0; i < te; ++i) sum[origins[q] + i] += w[i];
    weights.resize((size_t)k * te);
    for (int q = 0; q < k; ++q)
        for (int i = 0; i < te; ++i) weights[(size_t)q * te + i] = (float)(w[i] / sum[origins[q] + i]);  // one cover: w / w = 1 exactly
    return 0;
}

namespace {
inline int tile_blocks(long long work) { return (int)std::min<long long>((work + 255) / 256, 2048); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// xt[(b*T + ty*kx + tx), c, i, j] = x[b, c, oy[ty] + i, ox[tx] + j]; one thread per V elements of a tile row
template <int V>
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ x, float* __restrict__ xt, const int* __restrict__ oy,
                                                          const int* __restrict__ ox, int C, int H, int W, int ky, int kx, int th, int tw,
                                                          long long total) {
    const int twv = tw / V;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int jv = (int)(i % twv);
        long long q = i / twv;
        const int ii = (int)(q % th); q /= th;
        const int c = (int)(q % C); q /= C;
        const int T = ky * kx;
        const int ti = (int)(q % T);
        const long long b = q / T;
        const int ty = ti / kx, tx = ti % kx;
        const size_t src = (((size_t)b * C + c) * H + oy[ty] + ii) * W + ox[tx] + jv * V;
        if (V == 4) *reinterpret_cast<f32x4*>(xt + i * 4) = *reinterpret_cast<const f32x4*>(x + src);
        else xt[i] = x[src];
    }
}

// eps[b, c, y, x] = sum over the covering (ty, tx), ty ascending then tx ascending, of (nwy[ty][y - oy[ty]] * nwx[tx][x - ox[tx]]) * et[...];
// a gather per canvas element: fixed order, no atomics.  One thread per V canvas elements of a row (V = 4: the x origins and t_w are multiples
// of 4, so the four share their covering tiles).  The first term starts the sum, so a lone tile of weight 1 hands its bits through.
template <int V>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ et, float* __restrict__ eps, const int* __restrict__ oy,
                                                         const int* __restrict__ ox, const float* __restrict__ nwy,
                                                         const float* __restrict__ nwx, int C, int H, int W, int ky, int kx, int th, int tw,
                                                         long long total) {
    const int Wv = W / V;
    const int T = ky * kx;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int xx = (int)(i % Wv) * V;
        long long q = i / Wv;
        const int y = (int)(q % H); q /= H;
        const int c = (int)(q % C);
        const long long b = q / C;
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.f;
        bool first = true;
        for (int ty = 0; ty < ky; ++ty) {
            const int ly = y - oy[ty];
            if (ly < 0 || ly >= th) continue;
            const float wy = nwy[ty * th + ly];
            for (int tx = 0; tx < kx; ++tx) {
                const int lx = xx - ox[tx];
                if (lx < 0 || lx >= tw) continue;
                const size_t src = ((((size_t)b * T + ty * kx + tx) * C + c) * th + ly) * tw + lx;
                float e[V], wx[V];
                if (V == 4) {
                    const f32x4 ev = *reinterpret_cast<const f32x4*>(et + src);
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(nwx + tx * tw + lx);
#pragma unroll
                    for (int v = 0; v < V; ++v) { e[v] = ev[v]; wx[v] = wv[v]; }
                } else {
                    e[0] = et[src]; wx[0] = nwx[tx * tw + lx];
                }
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float term = (wy * wx[v]) * e[v];
                    acc[v] = first ? term : acc[v] + term;
                }
                first = false;
            }
        }
        if (V == 4) *reinterpret_cast<f32x4*>(eps + i * 4) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        else eps[i] = acc[0];
    }
}
}  // namespace

int launch_tile_gather(const float* x, float* xt, const TileGrid& g, int NB, int C, hipStream_t st) {
    const long long n = (long long)NB * g.ky * g.kx * C * g.th * g.tw;
    ProfScope ps("tile_gather", 0.0, 8.0 * n, st);
    if (g.vec4 && aligned16(x) && aligned16(xt)) {
        const long long total = n / 4;
        hipLaunchKernelGGL(tile_gather_kernel<4>, dim3(tile_blocks(total)), dim3(256), 0, st, x, xt, g.oy, g.ox, C, g.H, g.W, g.ky, g.kx, g.th,
                           g.tw, total);
    } else {
        hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(tile_blocks(n)), dim3(256), 0, st, x, xt, g.oy, g.ox, C, g.H, g.W, g.ky, g.kx, g.th,
                           g.tw, n);
    }
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_tile_blend(const float* et, float* eps, const TileGrid& g, int NB, int C, hipStream_t st) {
    const long long n = (long long)NB * C * g.H * g.W;
    ProfScope ps("tile_blend", 0.0, 4.0 * (n + (double)NB * g.ky * g.kx * C * g.th * g.tw), st);
    if (g.vec4 && aligned16(et) && aligned16(eps) && aligned16(g.nwx)) {
        const long long total = n / 4;
        hipLaunchKernelGGL(tile_blend_kernel<4>, dim3(tile_blocks(total)), dim3(256), 0, st, et, eps, g.oy, g.ox, g.nwy, g.nwx, C, g.H, g.W,
                           g.ky, g.kx, g.th, g.tw, total);
    } else {
        hipLaunchKernelGGL(tile_blend_kernel<1>, dim3(tile_blocks(n)), dim3(256), 0, st, et, eps, g.oy, g.ox, g.nwy, g.nwx, C, g.H, g.W, g.ky,
                           g.kx, g.th, g.tw, n);
    }
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

int TilePlan::build(int H_, int W_, int tile_h, int tile_w, int overlap_h, int overlap_w, int window) {
    H = H_; W = W_;
    TRY(tile_axis(H, tile_h, overlap_h, window, oy, nwy));
    TRY(tile_axis(W, tile_w, overlap_w, window, ox, nwx));
    th = std::min(tile_h, H); tw = std::min(tile_w, W);
    pack();
    return 0;
}
int TilePlan::check() {
    MRISR_REQUIRE(H > 0 && W > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "tiles: the tile must fit the canvas");
    auto axis = [](const std::vector<int>& o, int n, int t) {  // first at 0, last ending at n, increasing, no gap: every read and write in range
        if (o.empty() || o.front() != 0 || o.back() + t != n) return false;
        for (size_t i = 1; i < o.size(); ++i)
            if (o[i] <= o[i - 1] || o[i] - o[i - 1] > t) return false;
        return true;
    };
    MRISR_REQUIRE(axis(oy, H, th), "tiles: y origins must start at 0, increase, leave no gap and end at H - tile_h");
    MRISR_REQUIRE(axis(ox, W, tw), "tiles: x origins must start at 0, increase, leave no gap and end at W - tile_w");
    MRISR_REQUIRE(nwy.size() == oy.size() * th && nwx.size() == ox.size() * tw, "tiles: weight tables must be [n_tiles][tile]");
    return 0;
}
void TilePlan::pack() {
    auto pad4 = [](size_t v) { return (v + 3) / 4 * 4; };
    off_nwy = pad4(oy.size() + ox.size());
    off_nwx = pad4(off_nwy + nwy.size());
    words.assign(off_nwx + nwx.size(), 0u);
    memcpy(&words[0], oy.data(), oy.size() * 4);
    memcpy(&words[oy.size()], ox.data(), ox.size() * 4);
    memcpy(&words[off_nwy], nwy.data(), nwy.size() * 4);
    memcpy(&words[off_nwx], nwx.data(), nwx.size() * 4);
}
TileGrid TilePlan::grid(const void* dev) const {
    TileGrid g;
    g.H = H; g.W = W; g.th = th; g.tw = tw; g.ky = (int)oy.size(); g.kx = (int)ox.size();
    const uint32_t* base = static_cast<const uint32_t*>(dev);
    g.oy = reinterpret_cast<const int*>(base);
    g.ox = reinterpret_cast<const int*>(base + oy.size());
    g.nwy = reinterpret_cast<const float*>(base + off_nwy);
    g.nwx = reinterpret_cast<const float*>(base + off_nwx);
    g.vec4 = tw % 4 == 0 && W % 4 == 0;
    for (int o : ox) g.vec4 = g.vec4 && o % 4 == 0;
    return g;
}

}  // namespace mrisr

extern "C" int mrisr_tile_tables(int extent, int tile, int overlap, int window, int* origins, float* weights, int* n_tiles) {
    API_BEGIN
    MRISR_REQUIRE(n_tiles, "tile tables: n_tiles must not be null");
    std::vector<int> o;
    std::vector<float> w;
    TRY(mrisr::tile_axis(extent, tile, overlap, window, o, w));
    *n_tiles = (int)o.size();
    if (origins) memcpy(origins, o.data(), o.size() * sizeof(int));
    if (weights) memcpy(weights, w.data(), w.size() * sizeof(float));
    return 0;
    API_END
}
