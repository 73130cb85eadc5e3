// Conditioning strength: a multi-tensor scaled add.  ONE launch adds up to COND_MAX_PAIRS residuals r_k to their
// targets x_k, each with its own factor:
//
//   x_k[j] = round_T( fma(f_k, r_k[j], x_k[j]) )        f_k = w_k * table[4 * (*step) + col]      (f32; the product rounded once)
//
// table: the sampler's conditioning table [n_steps][4] = {c, a, 0, 0} (c: ControlNet scale of the step, a: adapter scale), row *step read
// behind the load of the step counter with ordinary loads, uniform over the launch - other values replay the same captured graph.  A null
// table gives f_k = w_k.  w_k: 1, or the guess-mode weight of residual k.
//
// x_k is addressed through a row range: pair k holds `per` elements per batch row, the launch adds to rows [row_lo, row_hi) of x_k and r_k
// has row_hi - row_lo rows (guess mode under classifier-free guidance: the residuals of the B conditional rows land on rows [B, 2B) of the
// UNet's batch; rows outside the range are not touched).
//
// grid.y is the pair; grid.x strides over 16-byte pieces (4 f32 / 8 bf16), every element read and written by the same lane, and the lanes
// of workgroup 0 finish the elements after the last whole piece.  The 16-byte path is taken only when both pointers of the pair (x at
// row_lo) are 16-byte aligned; otherwise the pair runs element by element.  f = 1 gives the bits of add_inplace (fma(1, r, x) == x + r, one
// rounding to T); f = 0 leaves x as it was (x + 0 r, r finite).
#include <algorithm>
#include <cmath>

#include "api.h"
#include "prof.h"
#include "runtime.h"

namespace mrisr {

template <typename T>
__global__ __launch_bounds__(256) void cond_add_kernel(CondAddArgs a) {
    constexpr int VE = 16 / (int)sizeof(T);
    union Vec { uint4 q; T e[VE]; };
    const CondAddPair& p = a.pair[blockIdx.y];
    float f = p.w;
    if (a.table) f = __fmul_rn(p.w, a.table[4 * (size_t)(*a.step) + a.col]);
    T* x = static_cast<T*>(p.x) + (size_t)a.row_lo * p.per;
    const T* r = static_cast<const T*>(p.r);
    const long long n = (long long)(a.row_hi - a.row_lo) * p.per;
    const long long stride = (long long)gridDim.x * 256, t0 = blockIdx.x * 256ll + threadIdx.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
    if (!vec) {
        for (long long i = t0; i < n; i += stride) x[i] = from_f32<T>(fmaf(f, to_f32(r[i]), to_f32(x[i])));
        return;
    }
    const long long nv = n / VE;
    for (long long i = t0; i < nv; i += stride) {
        Vec u, v;
        u.q = reinterpret_cast<const uint4*>(x)[i];
        v.q = reinterpret_cast<const uint4*>(r)[i];
#pragma unroll
        for (int e = 0; e < VE; ++e) u.e[e] = from_f32<T>(fmaf(f, to_f32(v.e[e]), to_f32(u.e[e])));
        reinterpret_cast<uint4*>(x)[i] = u.q;
    }
    if (blockIdx.x == 0) {
        const long long i = nv * VE + threadIdx.x;  // fewer than VE elements are left
        if (i < n) x[i] = from_f32<T>(fmaf(f, to_f32(r[i]), to_f32(x[i])));
    }
}

template <typename T>
int launch_cond_add(const CondAddArgs& a, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    MRISR_REQUIRE(a.n_pairs >= 1 && a.n_pairs <= COND_MAX_PAIRS, "cond add: 1 .. 16 pairs per launch");
    MRISR_REQUIRE(a.row_lo >= 0 && a.row_hi > a.row_lo, "cond add: an empty or negative row range");
    if (a.table) MRISR_REQUIRE(a.step && a.col >= 0 && a.col <= 1 && (reinterpret_cast<uintptr_t>(a.table) & 3) == 0,
                               "cond add: a table needs the step counter and column 0 (c) or 1 (a)");
    long long most = 0;
    double bytes = 0.0;
    for (int k = 0; k < a.n_pairs; ++k) {
        const CondAddPair& p = a.pair[k];
        MRISR_REQUIRE(p.x && p.r && p.per > 0, "cond add: null operand or empty pair");
        MRISR_REQUIRE(((reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.r)) & (sizeof(T) - 1)) == 0,
                      "cond add: operands must be aligned to their element");
        MRISR_REQUIRE(std::isfinite(p.w), "cond add: weights must be finite");
        const long long n = (long long)(a.row_hi - a.row_lo) * p.per;
        most = std::max(most, n);
        bytes += 3.0 * (double)n * sizeof(T);
    }
    const long long pieces = (most + VE - 1) / VE;
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((pieces + 255) / 256, 1), 2048);
    ProfScope ps("cond_add", 0.0, bytes, st);
    hipLaunchKernelGGL(cond_add_kernel<T>, dim3(gx, (unsigned)a.n_pairs), dim3(256), 0, st, a);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template int launch_cond_add<float>(const CondAddArgs&, hipStream_t);
template int launch_cond_add<bf16>(const CondAddArgs&, hipStream_t);

// the checks a conditioning table passes before anything touches the device: 0, or the error code with the message naming row and field
int check_conditioning_rows(const float* rows, int n_rows) {
    static const char* const names[4] = {"controlnet scale (c)", "adapter scale (a)", "column 2", "column 3"};
    for (int i = 0; i < n_rows; ++i) {
        const float* r = rows + 4 * (size_t)i;
        for (int c = 0; c < 4; ++c)
            MRISR_REQUIRE(std::isfinite(r[c]), "conditioning: row " + std::to_string(i) + ": " + names[c] + " is not finite");
        for (int c = 2; c < 4; ++c)
            MRISR_REQUIRE(r[c] == 0.f, "conditioning: row " + std::to_string(i) + ": " + names[c] + " must be 0");
    }
    return 0;
}

// diffusers' guess-mode weights (ControlNetModel.forward): logspace(-1, 0, n_down + 1), the mid residual last at weight 1; in f32
void guess_mode_weights(int n_down, float* w) {
    const double step = n_down > 0 ? 1.0 / n_down : 0.0;  // the exponents as numpy's linspace forms them: start + k * step
    for (int k = 0; k < n_down; ++k) w[k] = (float)std::pow(10.0, -1.0 + (double)k * step);
    w[n_down] = 1.f;
}

}  // namespace mrisr
