// The two composite backward operations of the training step that are more than one launch - the weight gradient of a conv / linear and
// the input gradient of a 3x3 conv - as free functions: the UNet / ControlNet trainer (train.hip) and the T2I-Adapter (adapter.hip) call
// them on their arenas, the single-op entry points (capi_ops.hip: mrisr_op_conv_wgrad / mrisr_op_conv_dgrad) on scratch buffers of
// their own, so the parity tests run the trainers' code.
#pragma once
#include <functional>

#include "gemm_args.h"

namespace mrisr {

typedef std::function<void*(size_t)> TrainAllocFn;    // device scratch that lives until the caller's stream work is done; null = failure
typedef std::function<int(GemmArgs&)> TrainGemmFn;    // plans (and, unless dry, launches) one GEMM: Runner::run_gemm or its stand-in

// full-parameter training: weight / bias gradient of one conv or linear, accumulated into gW / gB (f32, PyTorch layouts).  One
// pixel-contraction GEMM per layer,  dW[co][tap * cin + ci] = sum_m dY^T[co][m] . im2col^T[tap * cin + ci][m]  (a linear / 1 x 1 conv is the
// ks = 1 case), then one scatter-add; db by column sums.
//   x: NHWC [xB][xH][xW][cin_src] (rows [M][cin_src] for a linear: xB = 1, xH = M, xW = 1); dY: rows [M][.] of pitch ldy, columns
//   col0 .. col0 + cout_src; the raw tensor is [cout][cin][ks][ks] with cout <= cout_src, cin <= cin_src (zero-padded layers).
template <typename T>
int conv_wgrad_run(hipStream_t st, bool dry, const TrainAllocFn& alloc, const TrainGemmFn& run_gemm, const void* x, int xB, int xH, int xW,
                   int cin_src, const void* dY, int ldy, int col0, int Ho, int Wo, int cout_src, int ks, int stride, float* gW, float* gB,
                   int cout, int cin, int geglu_half) {
    const int M = xB * Ho * Wo, Mpad = (M + 63) / 64 * 64, taps = ks * ks;
    const int ncol = (taps * cin_src + 3) & ~3;  // the GEMM's N in multiples of 4 (3-channel images: 27 -> 28, one zero column)
    T* dyT = static_cast<T*>(alloc((size_t)cout_src * Mpad * sizeof(T)));
    T* xT = static_cast<T*>(alloc((size_t)ncol * Mpad * sizeof(T)));
    float* tmp = static_cast<float*>(alloc((size_t)cout_src * ncol * sizeof(float)));
    if (!dyT || !xT || !tmp) return 7;
    if (!dry) {
        // what the two fills below leave unwritten: the transpose the pixels M .. Mpad of dyT (the im2col zeroes its own), the im2col
        // the rows beyond taps * cin_src of xT
        if (Mpad != M) MRISR_CHECK_HIP(hipMemsetAsync(dyT, 0, (size_t)cout_src * Mpad * sizeof(T), st));
        if (ncol != taps * cin_src) MRISR_CHECK_HIP(hipMemsetAsync(xT, 0, (size_t)ncol * Mpad * sizeof(T), st));
        int rc = launch_transpose<T>(static_cast<const T*>(dY) + col0, dyT, M, cout_src, ldy, Mpad, 0, 0, 1, M, st);
        if (rc) return rc;
        if (gB && (rc = launch_colsum_gen<T>(dY, ldy, col0, gB, M, cout, geglu_half, st)) != 0) return rc;
        if ((rc = launch_im2col_all_T<T>(x, xT, xB, xH, xW, cin_src, Ho, Wo, stride, ks / 2, ks, Mpad, st)) != 0) return rc;
    }
    GemmArgs g;
    ga_rows(g, dyT, Mpad, Mpad); ga_weight(g, xT, cout_src, ncol, Mpad); ga_out_f32(g, tmp, ncol);
    if (int rc = run_gemm(g)) return rc;
    if (!dry && gW) return launch_wgrad_accum_gen(tmp, ncol, cin_src, gW, cout, cin, taps, geglu_half, st);
    return 0;
}

// dX = conv3x3(dY, wd) (+ resid), wd = the tap-flipped filter bank [cin][ky][kx][cout] (launch_pack_conv_dgrad).  dy: NHWC [B][H][W][cout];
// resid: rows of pitch ldr in out's shape, or null (resid == out accumulates in place).
// mode 1: the forward conv had stride 2 -> dY is zero-stuffed to twice its size.  Channel counts below one K tile take the direct kernel.
template <typename T>
int conv_dgrad_run(hipStream_t st, bool dry, const TrainGemmFn& run_gemm, const void* dy, int B, int H, int W, int cout, int cin,
                   const void* wd, int mode, void* out, const void* resid, int ldr) {
    constexpr int BK = 128 / (int)sizeof(T);
    const int Ho = H << mode, Wo = W << mode;
    if (cout % BK != 0 || cin % 4 != 0) {  // conv_out (4 channels): far below one K tile
        MRISR_REQUIRE(mode == 0 && (!resid || ldr == cin), "strided / pitched-residual dgrad of a tiny conv");
        DirectConvArgs a;
        a.x = dy; a.w = wd; a.y = out; a.B = B; a.Hin = H; a.Win = W; a.Cin = cout;
        a.Hout = Ho; a.Wout = Wo; a.Cout = cin; a.ks = 3; a.stride = 1; a.pad = 1; a.act = ACT_NONE;
        a.add = resid;
        if (dry) return 0;
        return launch_direct_conv<T>(a, st);
    }
    GemmArgs g;
    ga_rows(g, dy, cout, cout); ga_conv3(g, B, H, W, 1, mode, 1, mode); ga_weight(g, wd, B * Ho * Wo, cin, 9 * cout);
    if (resid) { ga_resid(g, resid, ldr); g.resid_exact = 1; }  // dX += ...: one rounding whatever kernel the planner picks
    ga_out(g, out, cin);
    return run_gemm(g);
}

}  // namespace mrisr
