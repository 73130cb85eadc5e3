// The test and bench surface of the C ABI (include/mrisr_debug.h, the mrisr_op_* part of include/mrisr.h): single-op entry points
// that run the very launchers the models use on caller buffers (parity tests), and the mrisr_bench_* micro-benchmarks.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "api.h"
#include "model.h"
#include "train_ops.h"

using namespace mrisr;

// =================================================================================================
// single-op entry points (parity tests drive the very kernels the models launch)
// =================================================================================================
namespace {
struct OpScratch {  // scratch of one call: freed when the entry returns (after its stream synchronisation)
    std::vector<std::unique_ptr<DevBuf>> bufs;
    void* alloc(size_t bytes, bool zero = false) {
        bufs.emplace_back(new DevBuf());
        if (bufs.back()->reserve(bytes ? bytes : 1, zero)) return nullptr;
        return bufs.back()->p;
    }
};
template <typename T>
int op_gemm_run(OpScratch& sc, hipStream_t st, GemmArgs& g) {  // Runner::run_gemm on scratch buffers
    return gemm_run<T>(g, st, false, [&sc](size_t n) { return sc.alloc(n); });
}
// honour a caller's split-K, else plan (a ForcedTile in scope applies either way); replan: with a split-K given, the planner still picks the
// tile.  The slabs come from `part`; the caller launches.
template <typename T>
int op_plan(GemmArgs& g, int splitk, bool replan, DevBuf& part) {
    g.splitk = splitk;
    if (splitk <= 0) { g.splitk = 1; TRY(gemm_choose(g, sizeof(T) == 2)); }
    else if (replan) { TRY(gemm_choose(g, sizeof(T) == 2)); g.splitk = splitk; }
    return gemm_alloc_partial(g, devbuf_alloc(part));
}
}  // namespace
template <typename T>
__global__ void rows_to_heads_kernel(const T* x, T* dst, int B, int N, int H, int hd, int npad, int dpad, int tr) {
    const long long total = (long long)B * N * H * hd;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int dd = (int)(i % hd);
        const int h = (int)((i / hd) % H);
        const int tok = (int)((i / ((long long)hd * H)) % N);
        const int b = (int)(i / ((long long)hd * H * N));
        const size_t bh = (size_t)b * H + h;
        if (!tr) dst[(bh * npad + tok) * dpad + dd] = x[i];
        else dst[(bh * dpad + dd) * npad + tok] = x[i];
    }
}

// test hook: mrisr_op_conv3x3 with stride 2 pads the low side with 0 instead of 1 (diffusers' Downsample2D(padding=0), asymmetric (0,1,0,1):
// the VAE encoder's down-sampler form, which no op reaches otherwise); even H and W, so the output shape is the same
static int g_op_conv_pad0 = 0;
extern "C" void mrisr_debug_op_conv_pad0(int on) { g_op_conv_pad0 = on; }

template <typename T>
static int op_conv3x3_t(const mrisr_tensor* x, const mrisr_tensor* x2, const float* w, const float* bias, int cout,
                        int stride, int ups, int act, int splitk, mrisr_tensor* y, hipStream_t st) {
    const int B = (int)x->shape[0], C0 = (int)x->shape[1], H = (int)x->shape[2], W = (int)x->shape[3];
    const int C1 = x2 ? (int)x2->shape[1] : 0;
    const int Cin = C0 + C1;
    DevBuf wp, part;
    TRY(wp.reserve((size_t)cout * Cin * 9 * sizeof(T), false));
    TRY(launch_pack_conv3x3<T>(w, wp.p, cout, Cin, 3, st));
    if (!x2 && !ups && Cin % (128 / (int)sizeof(T)) != 0) {
        // fan-in below one K tile (conv_in: 4 channels): the direct kernels (matrix-core conv_in form for bf16, 4 channels)
        DirectConvArgs a;
        a.x = x->data; a.w = wp.p; a.bias = bias; a.y = y->data; a.B = B; a.Hin = H; a.Win = W; a.Cin = Cin;
        a.Hout = (H - 1) / stride + 1; a.Wout = (W - 1) / stride + 1; a.Cout = cout; a.ks = 3; a.stride = stride; a.pad = 1; a.act = act;
        MRISR_REQUIRE(y->shape[1] == cout && y->shape[2] == a.Hout && y->shape[3] == a.Wout, "conv output shape");
        TRY(launch_direct_conv<T>(a, st));
        MRISR_CHECK_HIP(hipStreamSynchronize(st));
        return 0;
    }
    if (ups == 2) {  // the sub-pixel form of `nearest x2 -> conv3x3` (runner.h::upsample_conv): four 2 x 2 parity convs + interleave
        MRISR_REQUIRE(sizeof(T) == 2 && !x2 && stride == 1 && act == ACT_NONE && (4 * Cin) % 64 == 0 && cout % 8 == 0, "sub-pixel upsample conv: bf16, single source");
        MRISR_REQUIRE(y->shape[1] == cout && y->shape[2] == 2 * H && y->shape[3] == 2 * W, "conv output shape");
        DevBuf sp, planes;
        TRY(sp.reserve((size_t)16 * cout * Cin * sizeof(T), false));
        TRY(planes.reserve((size_t)4 * B * H * W * cout * sizeof(T), false));
        TRY(launch_pack_conv_subpix<T>(w, sp.p, cout, Cin, st));
        GemmArgs g;
        ga_rows(g, x->data, C0, C0); ga_conv3(g, B, H, W); g.kw = 2; g.subpix = 1;
        ga_batch(g, 4, 0, (long long)cout * 4 * Cin, (long long)B * H * W * cout); ga_weight(g, sp.p, B * H * W, cout, 4 * Cin);
        g.bias = bias; ga_out(g, planes.p, cout);
        TRY(gemm_run<T>(g, st, false, devbuf_alloc(part)));  // (un-split: a 2 x 2 conv takes no split-K)
        TRY(launch_subpix_shuffle<T>(planes.p, y->data, B, H, W, cout, st));
        MRISR_CHECK_HIP(hipStreamSynchronize(st));
        return 0;
    }
    GemmArgs g;
    ga_rows(g, x->data, C0, C0);
    if (x2) ga_rows2(g, x2->data, C1, C1);
    const bool pad0 = g_op_conv_pad0 && stride == 2 && !ups;
    if (pad0) MRISR_REQUIRE(H % 2 == 0 && W % 2 == 0, "stride-2 conv with pad 0: even H and W");
    ga_conv3(g, B, H, W, stride, ups, pad0 ? 0 : 1);
    MRISR_REQUIRE(y->shape[1] == cout && y->shape[2] == g.Hout && y->shape[3] == g.Wout, "conv output shape");
    ga_weight(g, wp.p, B * g.Hout * g.Wout, cout, 9 * Cin); g.bias = bias; g.act = act; ga_out(g, y->data, cout);
    TRY(op_plan<T>(g, splitk, false, part));
    TRY(launch_gemm<T>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" void mrisr_debug_force_tile(int t);
// one tile forced for the GEMMs of one op call: the planner is back when the scope ends, however it ends
struct ForcedTile {
    explicit ForcedTile(int t) { mrisr_debug_force_tile(t); }
    ~ForcedTile() { mrisr_debug_force_tile(0); }
    ForcedTile(const ForcedTile&) = delete;
    ForcedTile& operator=(const ForcedTile&) = delete;
};

// conv3x3(x) + bias + (W_sc [xs | xs2] + b_sc): a resnet's conv2 with its 1x1 conv_shortcut.  fused: ONE launch over K = [9 Cin | Cs] on the
// concatenated bank (the shortcut as the 1x1 tail of the K loop, summed bias); otherwise the two launches it replaces - the shortcut GEMM
// into y, then the conv with y as its residual in place.  `tile` picks the conv's kernel (the shortcut GEMM of the two-launch form is planned).
static int op_conv3x3_sc_t(const mrisr_tensor* x, const mrisr_tensor* x2, const float* w, const float* bias, const mrisr_tensor* xs,
                           const mrisr_tensor* xs2, const float* w_sc, const float* bias_sc, int cout, int splitk, int tile, int fused,
                           mrisr_tensor* y, hipStream_t st) {
    typedef bf16 T;
    const int B = (int)x->shape[0], C0 = (int)x->shape[1], H = (int)x->shape[2], W = (int)x->shape[3];
    const int C1 = x2 ? (int)x2->shape[1] : 0, Cin = C0 + C1;
    const int S0 = (int)xs->shape[1], S1 = xs2 ? (int)xs2->shape[1] : 0, Cs = S0 + S1;
    MRISR_REQUIRE(xs->shape[0] == B && xs->shape[2] == H && xs->shape[3] == W && (!xs2 || (xs2->shape[0] == B && xs2->shape[2] == H && xs2->shape[3] == W)),
                  "shortcut sources: the conv input's batch and image size");
    MRISR_REQUIRE(y->shape[1] == cout && y->shape[2] == H && y->shape[3] == W, "conv output shape");
    MRISR_REQUIRE(Cin % 64 == 0 && S0 % 64 == 0 && S1 % 64 == 0 && cout % 4 == 0, "channel counts: multiples of 64");
    const size_t K9 = (size_t)9 * Cin, Kt = K9 + Cs;
    DevBuf w9, wsc, bank, bsum, part;
    TRY(w9.reserve((size_t)cout * K9 * sizeof(T), false));
    TRY(wsc.reserve((size_t)cout * Cs * sizeof(T), false));
    TRY(launch_pack_conv3x3<T>(w, w9.p, cout, Cin, 3, st));
    TRY(launch_pack_rows<T>(w_sc, cout, Cs, wsc.p, Cs, 0, 0, 0, 0, 1.0f, st));
    GemmArgs g;
    ga_rows(g, x->data, C0, C0);
    if (x2) ga_rows2(g, x2->data, C1, C1);
    ga_conv3(g, B, H, W); ga_out(g, y->data, cout);
    const int M = B * H * W;
    if (fused) {
        TRY(bank.reserve((size_t)cout * Kt * sizeof(T), false));
        TRY(bsum.reserve((size_t)cout * sizeof(float), false));
        MRISR_CHECK_HIP(hipMemcpy2DAsync(bank.p, Kt * sizeof(T), w9.p, K9 * sizeof(T), K9 * sizeof(T), cout, hipMemcpyDeviceToDevice, st));
        MRISR_CHECK_HIP(hipMemcpy2DAsync(static_cast<T*>(bank.p) + K9, Kt * sizeof(T), wsc.p, (size_t)Cs * sizeof(T), (size_t)Cs * sizeof(T), cout,
                                         hipMemcpyDeviceToDevice, st));
        MRISR_CHECK_HIP(hipMemcpyAsync(bsum.p, bias, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, st));
        TRY(launch_add_inplace<float>(bsum.p, bias_sc, cout, st));
        ga_tail(g, xs->data, S0, S0);
        if (xs2) ga_tail2(g, xs2->data, S1, S1);
        ga_weight(g, bank.p, M, cout, (int)Kt); g.bias = static_cast<const float*>(bsum.p);
    } else {
        GemmArgs s;
        ga_rows(s, xs->data, S0, S0);
        if (xs2) ga_rows2(s, xs2->data, S1, S1);
        ga_weight(s, wsc.p, M, cout, Cs); s.bias = bias_sc; ga_out(s, y->data, cout);
        DevBuf spart;
        TRY(gemm_run<T>(s, st, false, devbuf_alloc(spart)));
        MRISR_CHECK_HIP(hipStreamSynchronize(st));
        ga_weight(g, w9.p, M, cout, (int)K9); g.bias = bias; ga_resid(g, y->data, cout);
    }
    ForcedTile forced(tile);
    TRY(op_plan<T>(g, splitk, !tile, part));
    TRY(launch_gemm<T>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// (h W2^T + b2 + t) Wp^T + bp + x: a transformer block's ff.net.2 followed by the transformer's proj_out.  fused: ONE launch over K = [K4 | C]
// on the composed bank [Wp W2 | Wp] (launch_compose_ff_proj), sources h and t, bias Wp b2 + bp, residual x; otherwise the two launches it
// replaces (the intermediate rounded to bf16).  Every launch is planned by gemm_choose (`tile` and mrisr_debug_force_split apply).
static int run_planned(GemmArgs& g, DevBuf& part, hipStream_t st) { return gemm_run<bf16>(g, st, false, devbuf_alloc(part)); }
static int op_ff_proj_t(const mrisr_tensor* h, const mrisr_tensor* t, const mrisr_tensor* x, const float* w2, const float* b2, const float* wp,
                        const float* bp, int tile, int fused, mrisr_tensor* y, hipStream_t st) {
    typedef bf16 T;
    const int M = (int)h->shape[0], K4 = (int)h->shape[1], C = (int)t->shape[1];
    MRISR_REQUIRE(t->shape[0] == M && x->shape[0] == M && x->shape[1] == C && y->shape[0] == M && y->shape[1] == C, "ff.net.2 + proj_out: row shapes");
    MRISR_REQUIRE(C % 64 == 0 && K4 % 64 == 0, "ff.net.2 + proj_out: widths that are multiples of 64");
    DevBuf bank, bsum, w2p, wpp, mid, part;
    if (fused) {
        const int Kt = K4 + C;
        TRY(bank.reserve((size_t)C * Kt * sizeof(T), false));
        TRY(bsum.reserve((size_t)C * sizeof(float), false));
        TRY(launch_compose_ff_proj(wp, w2, b2, bp, bank.p, Kt, static_cast<float*>(bsum.p), C, K4, st));
        TRY(launch_pack_rows<T>(wp, C, C, bank.p, Kt, 0, K4, 0, 0, 1.0f, st));
        GemmArgs g;
        ga_rows(g, h->data, K4, K4); ga_rows2(g, t->data, C, C); ga_weight(g, bank.p, M, C, Kt); g.bias = static_cast<const float*>(bsum.p);
        ga_resid(g, x->data, C); ga_out(g, y->data, C); g.no_rp = 1;
        ForcedTile forced(tile);
        TRY(run_planned(g, part, st));
    } else {
        TRY(w2p.reserve((size_t)C * K4 * sizeof(T), false));
        TRY(wpp.reserve((size_t)C * C * sizeof(T), false));
        TRY(mid.reserve((size_t)M * C * sizeof(T), false));
        TRY(launch_pack_rows<T>(w2, C, K4, w2p.p, K4, 0, 0, 0, 0, 1.0f, st));
        TRY(launch_pack_rows<T>(wp, C, C, wpp.p, C, 0, 0, 0, 0, 1.0f, st));
        GemmArgs g1, g2;
        auto linear = [&](GemmArgs& g, const void* a, int k, const void* w, const float* b, const void* resid, void* out) {
            ga_rows(g, a, k, k); ga_weight(g, w, M, C, k); g.bias = b; ga_resid(g, resid, C); ga_out(g, out, C);
        };
        linear(g1, h->data, K4, w2p.p, b2, t->data, mid.p);
        linear(g2, mid.p, C, wpp.p, bp, x->data, y->data);
        ForcedTile forced(tile);
        TRY(run_planned(g1, part, st));
        MRISR_CHECK_HIP(hipStreamSynchronize(st));  // (`part` is reused)
        TRY(run_planned(g2, part, st));
    }
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int op_attention_t(const mrisr_tensor* q, const mrisr_tensor* k, const mrisr_tensor* v, int H, int flash,
                          mrisr_tensor* out, hipStream_t st) {
    const int B = (int)q->shape[0], N = (int)q->shape[1], C = (int)q->shape[2], Nk = (int)k->shape[1];
    const int hd = C / H;
    constexpr int BK = 128 / (int)sizeof(T);
    const bool use_flash = flash && sizeof(T) == 2;
    const int dpad = round_up(hd, use_flash ? 32 : BK), npad = round_up(N, 64), nkpad = round_up(Nk, 64);
    DevBuf qb, kb, vb;
    TRY(qb.reserve((size_t)B * H * npad * dpad * sizeof(T), true));
    TRY(kb.reserve((size_t)B * H * nkpad * dpad * sizeof(T), true));
    TRY(vb.reserve((size_t)B * H * dpad * nkpad * sizeof(T), true));
    auto conv = [&](const mrisr_tensor* x, void* dst, int n, int np, int tr) {
        hipLaunchKernelGGL(rows_to_heads_kernel<T>, dim3(1024), dim3(256), 0, st, static_cast<const T*>(x->data),
                           static_cast<T*>(dst), B, n, H, hd, np, dpad, tr);
    };
    conv(q, qb.p, N, npad, 0);
    conv(k, kb.p, Nk, nkpad, 0);
    conv(v, vb.p, Nk, nkpad, 1);
    MRISR_CHECK_HIP(hipGetLastError());
    // from here on the core the models run (gemm_args.h), on scratch buffers
    OpScratch sc;
    auto scratch = [&sc](size_t n) { return sc.alloc(n); };
    AttnGeom geo;
    geo.B = B; geo.H = H; geo.N = N; geo.npad = npad; geo.hd = hd; geo.dpad = dpad; geo.nk = Nk; geo.nkpad = nkpad;
    if (use_flash) {
        const bool fp8 = flash == 2;  // fp8 (OCP e4m3) Q K^T and P V
        AttnArgs a;
        TRY(attn_flash_args(a, geo, qb.p, kb.p, vb.p, out->data, nullptr, fp8, scratch));
        TRY(attn_flash_launch(a, fp8, false, st));
    } else {
        const size_t cnt = (size_t)B * H * N * nkpad;
        float* S = static_cast<float*>(sc.alloc(cnt * sizeof(float)));
        void* P = sizeof(T) == 2 ? sc.alloc(cnt * sizeof(T)) : S;
        if (!S || !P) return 7;
        TRY(attn_materialised<T>(geo, qb.p, kb.p, vb.p, S, P, out->data, false, st, [&](GemmArgs& g) { return op_gemm_run<T>(sc, st, g); }));
    }
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}


// ---- LoRA on a 3x3 conv (lora_conv.hip): the adapter arrives as peft's f32 tensors and is packed here by the trainer's own packer ----
template <typename T>
static int op_conv_lora_down_t(const void* x, int B, int H, int W, int cin, const float* A, int r, float* z, int route, hipStream_t st) {
    DevBuf av, bdummy, scr;
    TRY(av.reserve((size_t)r * 9 * cin * sizeof(T), false));
    TRY(bdummy.reserve((size_t)r * sizeof(float), true));  // (a [1][r] B: the packer takes both tensors)
    TRY(launch_conv_lora_pack<T>(A, static_cast<const float*>(bdummy.p), 1.0f, av.p, nullptr, nullptr, nullptr, cin, 1, r, st));
    const size_t sb = conv_lora_down_scratch_bytes(B * H * W, cin, r, sizeof(T), route);
    if (sb) TRY(scr.reserve(sb, false));
    TRY(launch_conv_lora_down<T>(x, av.p, z, B, H, W, cin, r, static_cast<float*>(scr.p), st, route));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}
template <typename T>
static int op_conv_lora_dgrad_t(const float* dz, int B, int H, int W, int r, const float* A, int cin, void* dx, int accumulate, hipStream_t st) {
    DevBuf av, bank, bdummy;
    TRY(av.reserve((size_t)r * 9 * cin * sizeof(T), false));
    if (sizeof(T) == 2) TRY(bank.reserve((size_t)cin * conv_lora_kpad(r) * 2, true));
    TRY(bdummy.reserve((size_t)r * sizeof(float), true));
    TRY(launch_conv_lora_pack<T>(A, static_cast<const float*>(bdummy.p), 1.0f, av.p, bank.p, nullptr, nullptr, cin, 1, r, st));
    TRY(launch_conv_lora_dgrad<T>(dz, av.p, bank.p, dx, B, H, W, cin, r, accumulate, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}
// conv3x3(x) + bias + rowvec[image] + s B conv3x3(x, A) + resid: the down-projection kernel, then the conv GEMM with the rank-r term in its
// epilogue - the two launches of an adapted resnet conv (runner.h::conv_lora_z / conv3)
template <typename T>
static int op_conv3x3_lora_t(const mrisr_tensor* x, const float* w, const float* bias, const float* A, const float* Bm, int r, float scale,
                             const float* rowvec, const mrisr_tensor* resid, int cout, int splitk, int tile, mrisr_tensor* y, hipStream_t st) {
    const int B = (int)x->shape[0], Cin = (int)x->shape[1], H = (int)x->shape[2], W = (int)x->shape[3], M = B * H * W;
    DevBuf wp, av, sb, zb, scr, part;
    TRY(wp.reserve((size_t)cout * Cin * 9 * sizeof(T), false));
    TRY(launch_pack_conv3x3<T>(w, wp.p, cout, Cin, 3, st));
    if (r > 0) {  // (r = 0: the conv with its row vector and residual alone)
        TRY(av.reserve((size_t)r * 9 * Cin * sizeof(T), false));
        TRY(sb.reserve((size_t)cout * r * sizeof(float), false));
        TRY(zb.reserve((size_t)M * r * sizeof(float), false));
        TRY(launch_conv_lora_pack<T>(A, Bm, scale, av.p, nullptr, static_cast<float*>(sb.p), nullptr, Cin, cout, r, st));
        const size_t sbytes = conv_lora_down_scratch_bytes(M, Cin, r, sizeof(T));
        if (sbytes) TRY(scr.reserve(sbytes, false));
        TRY(launch_conv_lora_down<T>(x->data, av.p, static_cast<float*>(zb.p), B, H, W, Cin, r, static_cast<float*>(scr.p), st));
    }
    GemmArgs g;
    ga_rows(g, x->data, Cin, Cin); ga_conv3(g, B, H, W); ga_weight(g, wp.p, M, cout, 9 * Cin); g.bias = bias;
    if (rowvec) ga_rowvec(g, rowvec, cout, H * W);
    if (resid) ga_resid(g, resid->data, cout);
    ga_out(g, y->data, cout);
    if (r > 0) ga_lora_epilogue(g, static_cast<const float*>(zb.p), r, static_cast<const float*>(sb.p), r, cout);
    ForcedTile forced(tile);
    TRY(op_plan<T>(g, splitk, !tile, part));
    TRY(launch_gemm<T>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// y = act(x W^T + bias) on row tensors (K = x's width, the output pitch y's)
static GemmArgs op_linear_args(const mrisr_tensor* x, const void* w, int n, const float* bias, int act, const mrisr_tensor* y) {
    const int K = (int)x->shape[1];
    GemmArgs g;
    ga_rows(g, x->data, K, K); ga_weight(g, w, (int)x->shape[0], n, K); g.bias = bias; g.act = act; ga_out(g, y->data, (int)y->shape[1]);
    return g;
}

extern "C" {

static int op_dtype_ok(const mrisr_tensor* x) {
    MRISR_REQUIRE(x && (x->dtype == MRISR_F32 || x->dtype == MRISR_BF16), "op tensors: f32 or bf16");
    return 0;
}

int mrisr_op_conv3x3(const mrisr_tensor* x, const mrisr_tensor* x2, const float* w_oihw_dev, const float* bias_dev,
                     int cout, int stride, int upsample, int act, int splitk, int tile, mrisr_tensor* y,
                     void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    TRY(gemm_prepare());
    MRISR_REQUIRE(x->layout == MRISR_NHWC && y && y->layout == MRISR_NHWC && y->dtype == x->dtype, "NHWC in/out, same dtype");
    ForcedTile forced(tile);
    return x->dtype == MRISR_F32 ? op_conv3x3_t<float>(x, x2, w_oihw_dev, bias_dev, cout, stride, upsample, act, splitk, y, (hipStream_t)stream)
                                 : op_conv3x3_t<bf16>(x, x2, w_oihw_dev, bias_dev, cout, stride, upsample, act, splitk, y, (hipStream_t)stream);
    API_END
}

int mrisr_op_conv3x3_sc(const mrisr_tensor* x, const mrisr_tensor* x2, const float* w_oihw_dev, const float* bias_dev, const mrisr_tensor* xs,
                        const mrisr_tensor* xs2, const float* w_sc_dev, const float* bias_sc_dev, int cout, int splitk, int tile, int fused,
                        mrisr_tensor* y, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && xs && y && w_oihw_dev && bias_dev && w_sc_dev && bias_sc_dev, "null argument");
    MRISR_REQUIRE(x->dtype == MRISR_BF16 && xs->dtype == MRISR_BF16 && y->dtype == MRISR_BF16 && (!x2 || x2->dtype == MRISR_BF16) &&
                      (!xs2 || xs2->dtype == MRISR_BF16),
                  "conv3x3 + 1x1 shortcut: bf16 tensors");
    MRISR_REQUIRE(x->layout == MRISR_NHWC && xs->layout == MRISR_NHWC && y->layout == MRISR_NHWC && (!x2 || x2->layout == MRISR_NHWC) &&
                      (!xs2 || xs2->layout == MRISR_NHWC),
                  "NHWC in/out");
    TRY(gemm_prepare());
    return op_conv3x3_sc_t(x, x2, w_oihw_dev, bias_dev, xs, xs2, w_sc_dev, bias_sc_dev, cout, splitk, tile, fused, y, (hipStream_t)stream);
    API_END
}

int mrisr_op_ff_proj(const mrisr_tensor* h, const mrisr_tensor* t, const mrisr_tensor* x, const float* w2_dev, const float* b2_dev,
                     const float* wp_dev, const float* bp_dev, int tile, int fused, mrisr_tensor* y, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(h && t && x && y && w2_dev && wp_dev, "null argument");
    MRISR_REQUIRE(h->dtype == MRISR_BF16 && t->dtype == MRISR_BF16 && x->dtype == MRISR_BF16 && y->dtype == MRISR_BF16, "ff.net.2 + proj_out: bf16 rows");
    MRISR_REQUIRE(h->ndim == 2 && t->ndim == 2 && x->ndim == 2 && y->ndim == 2, "rows in/out");
    TRY(gemm_prepare());
    return op_ff_proj_t(h, t, x, w2_dev, b2_dev, wp_dev, bp_dev, tile, fused, y, (hipStream_t)stream);
    API_END
}

int mrisr_op_linear(const mrisr_tensor* x, const float* w_dev, const float* bias_dev, int n, int act, int splitk,
                    int tile, mrisr_tensor* y, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    TRY(gemm_prepare());
    MRISR_REQUIRE(x->ndim == 2 && y && y->ndim == 2 && y->dtype == x->dtype, "rows in/out");
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], K = (int)x->shape[1];
    const bool f32 = x->dtype == MRISR_F32;
    const int esz = f32 ? 4 : 2;
    DevBuf wp, part, bp;
    TRY(wp.reserve((size_t)n * K * esz, false));
    const bool geglu = act == ACT_GEGLU;
    if (f32) TRY(launch_pack_rows<float>(w_dev, n, K, wp.p, K, 0, 0, geglu ? 1 : 0, n / 2, 1.0f, st));
    else TRY(launch_pack_rows<bf16>(w_dev, n, K, wp.p, K, 0, 0, geglu ? 1 : 0, n / 2, 1.0f, st));
    const float* bias = bias_dev;
    if (geglu && bias_dev) {
        TRY(bp.reserve((size_t)n * sizeof(float), false));
        TRY(launch_pack_bias_geglu(bias_dev, static_cast<float*>(bp.p), n / 2, st));
        bias = static_cast<const float*>(bp.p);
    }
    GemmArgs g = op_linear_args(x, wp.p, n, bias, act, y);
    ForcedTile forced(tile);
    TRY(f32 ? op_plan<float>(g, splitk, false, part) : op_plan<bf16>(g, splitk, false, part));
    TRY(f32 ? launch_gemm<float>(g, st) : launch_gemm<bf16>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// y = x W^T + bias + rowvec[m / (M / rowvec_rows)] + s B (A x) + resid on bf16 rows: a projection with everything its epilogue can carry, as
// Runner::linear builds it (the adapter's z = x A^T inside the kernel where the tile computes it, else by launch_lora_down).  resid may be y.
int mrisr_op_linear_resid(const mrisr_tensor* x, const float* w_dev, const float* bias_dev, int n, const float* rowvec_dev, int rowvec_rows,
                          const float* lora_a_dev, const float* lora_b_dev, int lora_r, float lora_scale, const mrisr_tensor* resid, int splitk,
                          int tile, mrisr_tensor* y, void* stream) {
    API_BEGIN
    typedef bf16 T;
    MRISR_REQUIRE(x && y && w_dev && x->dtype == MRISR_BF16 && y->dtype == MRISR_BF16 && x->ndim == 2 && y->ndim == 2, "linear + residual: bf16 rows in/out");
    MRISR_REQUIRE(!resid || (resid->dtype == MRISR_BF16 && resid->ndim == 2 && resid->shape[0] == x->shape[0] && resid->shape[1] >= n), "residual rows");
    TRY(gemm_prepare());
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], K = (int)x->shape[1];
    MRISR_REQUIRE(!rowvec_dev || (rowvec_rows >= 1 && M % rowvec_rows == 0), "row vector: rows dividing M");
    MRISR_REQUIRE(lora_r == 0 || (lora_r >= 1 && lora_r <= 16 && lora_a_dev && lora_b_dev && splitk <= 1), "adapter: rank 1 .. 16, A and B, un-split");
    DevBuf wp, part, av, sb, zb;
    TRY(wp.reserve((size_t)n * K * sizeof(T), false));
    TRY(launch_pack_rows<T>(w_dev, n, K, wp.p, K, 0, 0, 0, 0, 1.0f, st));
    GemmArgs g = op_linear_args(x, wp.p, n, bias_dev, ACT_NONE, y);
    if (rowvec_dev) ga_rowvec(g, rowvec_dev, n, M / rowvec_rows);
    if (resid) ga_resid(g, resid->data, (int)resid->shape[1]);
    ForcedTile forced(tile);
    if (!lora_r) {
        TRY(op_plan<T>(g, splitk, false, part));
    } else {
        TRY(av.reserve((size_t)lora_r * K * sizeof(T), false));
        TRY(sb.reserve((size_t)n * lora_r * sizeof(float), false));
        TRY(zb.reserve((size_t)M * lora_r * sizeof(float), false));
        TRY(launch_pack_rows<T>(lora_a_dev, lora_r, K, av.p, K, 0, 0, 0, 0, 1.0f, st));
        TRY(launch_pack_rows<float>(lora_b_dev, n, lora_r, sb.p, lora_r, 0, 0, 0, 0, lora_scale, st));
        ga_lora_epilogue(g, nullptr, lora_r, static_cast<const float*>(sb.p), lora_r, n);
        g.no_rp = 1;
        TRY(op_plan<T>(g, 0, false, part));
        if (g.splitk == 1 && gemm_tile_lora_in_kernel(g.tile, lora_r, lora_r)) {
            g.lora_a = av.p; g.lora_R = lora_r;
        } else {
            TRY(launch_lora_down<T>(x->data, K, av.p, static_cast<float*>(zb.p), M, K, lora_r, st));
            g.lora_z = static_cast<const float*>(zb.p);
        }
    }
    TRY(launch_gemm<T>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_ln_linear(const mrisr_tensor* x, const float* gamma_dev, const float* beta_dev, const float* w_dev, const float* bias_dev,
                       int n, int act, mrisr_tensor* y, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    TRY(gemm_prepare());
    MRISR_REQUIRE(x->ndim == 2 && y && y->ndim == 2 && y->dtype == x->dtype && x->dtype == MRISR_BF16, "bf16 rows in/out");
    MRISR_REQUIRE(gamma_dev && beta_dev && w_dev, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], K = (int)x->shape[1];
    DevBuf wp, bp;
    TRY(wp.reserve((size_t)n * K * 2, false));
    const bool geglu = act == ACT_GEGLU;
    TRY(launch_pack_rows<bf16>(w_dev, n, K, wp.p, K, 0, 0, geglu ? 1 : 0, n / 2, 1.0f, st));
    const float* bias = bias_dev;
    if (geglu && bias_dev) {
        TRY(bp.reserve((size_t)n * sizeof(float), false));
        TRY(launch_pack_bias_geglu(bias_dev, static_cast<float*>(bp.p), n / 2, st));
        bias = static_cast<const float*>(bp.p);
    }
    GemmArgs g = op_linear_args(x, wp.p, n, bias, act, y);
    MRISR_REQUIRE(gemm_rp_tile(g) != 0, "LayerNorm prologue: the row-panel kernel does not take this shape (K = 320 / 640, N % 16 == 0)");
    g.ln_gamma = gamma_dev; g.ln_beta = beta_dev; g.ln_eps = 1e-5f;
    TRY(gemm_choose(g, true));
    TRY(launch_gemm<bf16>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_mlp(const mrisr_tensor* x, const float* gamma_dev, const float* beta_dev, const float* w1_dev, const float* b1_dev,
                 const float* w2_dev, const float* b2_dev, int hidden, int residual, mrisr_tensor* y, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    TRY(gemm_prepare());
    MRISR_REQUIRE(x->ndim == 2 && y && y->ndim == 2 && y->dtype == x->dtype && x->dtype == MRISR_BF16, "bf16 rows in/out");
    MRISR_REQUIRE(gamma_dev && beta_dev && w1_dev && w2_dev, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], C = (int)x->shape[1], N2 = (int)y->shape[1];
    MRISR_REQUIRE(y->shape[0] == M && mlp_fused_ok(C, hidden, N2), "fused feed-forward: C = 320 rows in and out, hidden % 32 == 0");
    DevBuf w1p, b1p, w2b, w2p;
    TRY(w1p.reserve((size_t)2 * hidden * C * 2, false));
    TRY(w2b.reserve((size_t)N2 * hidden * 2, false));
    TRY(w2p.reserve((size_t)N2 * hidden * 2, false));
    TRY(launch_pack_rows<bf16>(w1_dev, 2 * hidden, C, w1p.p, C, 0, 0, 1, hidden, 1.0f, st));
    TRY(launch_pack_rows<bf16>(w2_dev, N2, hidden, w2b.p, hidden, 0, 0, 0, 0, 1.0f, st));
    TRY(launch_pack_mlp_w2(w2b.p, w2p.p, N2, hidden, st));
    const float* b1 = nullptr;
    if (b1_dev) {
        TRY(b1p.reserve((size_t)2 * hidden * sizeof(float), false));
        TRY(launch_pack_bias_geglu(b1_dev, static_cast<float*>(b1p.p), hidden, st));
        b1 = static_cast<const float*>(b1p.p);
    }
    MlpArgs a;
    a.x = x->data; a.ldx = C; a.M = M; a.ln_gamma = gamma_dev; a.ln_beta = beta_dev; a.ln_eps = 1e-5f;
    a.w1 = w1p.p; a.b1 = b1; a.w2p = w2p.p; a.b2 = b2_dev;
    a.resid = residual ? x->data : nullptr; a.ldr = C; a.out = y->data; a.ldo = N2; a.C = C; a.H = hidden; a.N2 = N2;
    TRY(launch_mlp_fused(a, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_mlp_proj(const mrisr_tensor* x, const float* gamma_dev, const float* beta_dev, const float* w1_dev, const float* b1_dev,
                      const float* w2_dev, const float* b2_dev, int hidden, int residual, const float* wp_dev, const float* bp_dev,
                      const mrisr_tensor* xres, mrisr_tensor* y, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(x && xres && y && gamma_dev && beta_dev && w1_dev && w2_dev && wp_dev, "null argument");
    MRISR_REQUIRE(x->dtype == MRISR_BF16 && xres->dtype == MRISR_BF16 && y->dtype == MRISR_BF16 && x->ndim == 2 && xres->ndim == 2 && y->ndim == 2,
                  "bf16 rows in/out");
    TRY(gemm_prepare());
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], C = (int)x->shape[1];
    MRISR_REQUIRE(mlp_fused_ok(C, hidden, C), "fused feed-forward: C = 320 rows in and out, hidden % 32 == 0");
    MRISR_REQUIRE(xres->shape[0] == M && xres->shape[1] == C && y->shape[0] == M && y->shape[1] == C, "fused feed-forward + proj_out: row shapes");
    MRISR_REQUIRE(M > 0 && M % 128 == 0, "fused feed-forward + proj_out: whole 128-row panels");
    DevBuf w1p, b1p, w2b, w2p, wpb, wpp, ff;
    TRY(w1p.reserve((size_t)2 * hidden * C * 2, false));
    TRY(w2b.reserve((size_t)C * hidden * 2, false));
    TRY(w2p.reserve((size_t)C * hidden * 2, false));
    TRY(wpb.reserve((size_t)C * C * 2, false));
    TRY(wpp.reserve((size_t)C * C * 2, false));
    TRY(ff.reserve((size_t)M * C * 2, false));  // (MlpArgs::out: required, never stored in this form)
    TRY(launch_pack_rows<bf16>(w1_dev, 2 * hidden, C, w1p.p, C, 0, 0, 1, hidden, 1.0f, st));
    TRY(launch_pack_rows<bf16>(w2_dev, C, hidden, w2b.p, hidden, 0, 0, 0, 0, 1.0f, st));
    TRY(launch_pack_mlp_w2(w2b.p, w2p.p, C, hidden, st));
    TRY(launch_pack_rows<bf16>(wp_dev, C, C, wpb.p, C, 0, 0, 0, 0, 1.0f, st));
    TRY(launch_pack_mlp_w2(wpb.p, wpp.p, C, C, st));
    const float* b1 = nullptr;
    if (b1_dev) {
        TRY(b1p.reserve((size_t)2 * hidden * sizeof(float), false));
        TRY(launch_pack_bias_geglu(b1_dev, static_cast<float*>(b1p.p), hidden, st));
        b1 = static_cast<const float*>(b1p.p);
    }
    MlpArgs a;
    a.x = x->data; a.ldx = C; a.M = M; a.ln_gamma = gamma_dev; a.ln_beta = beta_dev; a.ln_eps = 1e-5f;
    a.w1 = w1p.p; a.b1 = b1; a.w2p = w2p.p; a.b2 = b2_dev;
    a.resid = residual ? x->data : nullptr; a.ldr = C; a.out = ff.p; a.ldo = C; a.C = C; a.H = hidden; a.N2 = C;
    a.wp = wpp.p; a.bp = bp_dev; a.xres = xres->data; a.ldxr = C; a.out2 = y->data; a.ldo2 = C;
    TRY(launch_mlp_fused(a, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_xattn_tail(const mrisr_tensor* ao, mrisr_tensor* t, int ntok, const float* w1_dev, const float* b1_dev, const float* gamma_dev,
                        const float* beta_dev, const float* wq_dev, const float* bq_dev, const float* w2_dev, const float* b2_dev,
                        const mrisr_tensor* k, const mrisr_tensor* v, int nk, const float* a1_dev, const float* lb1_dev, const float* aq_dev,
                        const float* lbq_dev, const float* a2_dev, const float* lb2_dev, int lora_r, float lora_scale, void* stream) {
    API_BEGIN
    typedef bf16 T;
    constexpr int C = 320, H = 8, hd = 40;
    MRISR_REQUIRE(ao && t && k && v && w1_dev && gamma_dev && beta_dev && wq_dev && w2_dev, "null argument");
    MRISR_REQUIRE(ao->dtype == MRISR_BF16 && t->dtype == MRISR_BF16 && k->dtype == MRISR_BF16 && v->dtype == MRISR_BF16, "xattn tail: bf16 rows");
    MRISR_REQUIRE(ao->ndim == 2 && t->ndim == 2 && k->ndim == 3 && v->ndim == 3, "xattn tail: ao, t [M][ld]; k, v [B][keys][320]");
    const int M = (int)ao->shape[0], ldao = (int)ao->shape[1], ldt = (int)t->shape[1], B = (int)k->shape[0], nkbuf = (int)k->shape[1];
    MRISR_REQUIRE(t->shape[0] == M && ldao >= C && ldt >= C && ldao % 8 == 0 && ldt % 8 == 0, "xattn tail: row shapes (pitches >= 320, multiples of 8)");
    MRISR_REQUIRE(ntok > 0 && xattn_tail_ok(C, H, M, ntok, nk), "xattn tail: C = 320, 8 heads, whole 128-row panels inside one image, 1 .. 80 keys");
    MRISR_REQUIRE(B == M / ntok && k->shape[2] == C && v->shape[0] == B && v->shape[1] == nkbuf && v->shape[2] == C && nk <= nkbuf,
                  "xattn tail: k, v [M / ntok][>= nk][320]");
    const int nad = (a1_dev != nullptr) + (lb1_dev != nullptr) + (aq_dev != nullptr) + (lbq_dev != nullptr) + (a2_dev != nullptr) + (lb2_dev != nullptr);
    MRISR_REQUIRE((lora_r == 0 && nad == 0) || (lora_r == 4 && nad == 6), "xattn tail: rank-4 adapters on all three projections, or none");
    TRY(gemm_prepare());
    hipStream_t st = (hipStream_t)stream;
    // the packing of Packer::xf (model.hip) and Runner::project_context (runner.h), on buffers of this call
    const int dpad = 64, ctx_pad = round_up(nkbuf, 64);
    DevBuf w1p, wqb, wqp, w2b, w2p, kc, vtc, kvp, ab[3], lbb[3];
    TRY(w1p.reserve((size_t)C * C * sizeof(T), false));
    TRY(wqb.reserve((size_t)C * C * sizeof(T), false));
    TRY(wqp.reserve((size_t)C * C * sizeof(T), false));
    TRY(w2b.reserve((size_t)C * C * sizeof(T), false));
    TRY(w2p.reserve((size_t)C * C * sizeof(T), false));
    TRY(kc.reserve((size_t)B * H * ctx_pad * dpad * sizeof(T), true));
    TRY(vtc.reserve((size_t)B * H * dpad * ctx_pad * sizeof(T), true));
    TRY(kvp.reserve(xattn_tail_kv_bytes(B), false));
    TRY(launch_pack_rows<T>(w1_dev, C, C, w1p.p, C, 0, 0, 0, 0, 1.0f, st));
    TRY(launch_pack_rows<T>(wq_dev, C, C, wqb.p, C, 0, 0, 0, 0, 1.0f, st));
    TRY(launch_pack_rows<T>(w2_dev, C, C, w2b.p, C, 0, 0, 0, 0, 1.0f, st));
    TRY(launch_pack_mlp_w2(wqb.p, wqp.p, C, C, st));
    TRY(launch_pack_mlp_w2(w2b.p, w2p.p, C, C, st));
    hipLaunchKernelGGL(rows_to_heads_kernel<T>, dim3(1024), dim3(256), 0, st, static_cast<const T*>(k->data), static_cast<T*>(kc.p), B, nkbuf, H, hd,
                       ctx_pad, dpad, 0);
    hipLaunchKernelGGL(rows_to_heads_kernel<T>, dim3(1024), dim3(256), 0, st, static_cast<const T*>(v->data), static_cast<T*>(vtc.p), B, nkbuf, H, hd,
                       ctx_pad, dpad, 1);
    MRISR_CHECK_HIP(hipGetLastError());
    TRY(launch_pack_xattn_kv(kc.p, vtc.p, kvp.p, B, ctx_pad, dpad, nk, st));
    if (lora_r) {
        const float* A[3] = {a1_dev, aq_dev, a2_dev};
        const float* Bm[3] = {lb1_dev, lbq_dev, lb2_dev};
        for (int i = 0; i < 3; ++i) {
            TRY(ab[i].reserve((size_t)lora_r * C * sizeof(T), false));
            TRY(lbb[i].reserve((size_t)C * lora_r * sizeof(float), false));
            TRY(launch_pack_rows<T>(A[i], lora_r, C, ab[i].p, C, 0, 0, 0, 0, 1.0f, st));
            TRY(launch_pack_rows<float>(Bm[i], C, lora_r, lbb[i].p, lora_r, 0, 0, 0, 0, lora_scale, st));
        }
    }
    XTailArgs a;
    a.ao = ao->data; a.ldao = ldao; a.t = t->data; a.ldt = ldt; a.M = M; a.ntok = ntok;
    a.w1 = w1p.p; a.b1 = b1_dev; a.a1 = ab[0].p; a.lb1 = static_cast<const float*>(lbb[0].p);
    a.ln_g = gamma_dev; a.ln_b = beta_dev; a.ln_eps = 1e-5f;
    a.wq = wqp.p; a.bq = bq_dev; a.aq = ab[1].p; a.lbq = static_cast<const float*>(lbb[1].p);
    a.kvp = kvp.p; a.nk = nk; a.scale = 1.0f / sqrtf((float)hd);
    a.w2 = w2p.p; a.b2 = b2_dev; a.a2 = ab[2].p; a.lb2 = static_cast<const float*>(lbb[2].p);
    a.lora_r = lora_r;
    TRY(launch_xattn_tail(a, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_linear_fp8(const mrisr_tensor* x, const float* gamma_dev, const float* beta_dev, const float* w_dev, const float* bias_dev,
                        int n, int act, mrisr_tensor* y, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    TRY(gemm_prepare());
    MRISR_REQUIRE(x->ndim == 2 && y && y->ndim == 2 && y->dtype == x->dtype && x->dtype == MRISR_BF16 && w_dev, "bf16 rows in/out");
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], K = (int)x->shape[1];
    DevBuf wp, w8, ws, bp;
    TRY(wp.reserve((size_t)n * K * 2, false));
    TRY(w8.reserve((size_t)n * K, false));
    TRY(ws.reserve((size_t)n * sizeof(float), false));
    const bool geglu = act == ACT_GEGLU;
    TRY(launch_pack_rows<bf16>(w_dev, n, K, wp.p, K, 0, 0, geglu ? 1 : 0, n / 2, 1.0f, st));
    TRY(launch_quant_rows_fp8(wp.p, n, K, w8.p, static_cast<float*>(ws.p), st));
    const float* bias = bias_dev;
    if (geglu && bias_dev) {
        TRY(bp.reserve((size_t)n * sizeof(float), false));
        TRY(launch_pack_bias_geglu(bias_dev, static_cast<float*>(bp.p), n / 2, st));
        bias = static_cast<const float*>(bp.p);
    }
    GemmArgs g = op_linear_args(x, wp.p, n, bias, act, y);
    g.w8 = w8.p; g.w_scale = static_cast<const float*>(ws.p);
    MRISR_REQUIRE(gemm_rp_tile(g) != 0, "fp8 operands: the row-panel kernel does not take this shape (K = 320 / 640, N % 16 == 0)");
    if (gamma_dev) { g.ln_gamma = gamma_dev; g.ln_beta = beta_dev; g.ln_eps = 1e-5f; }
    TRY(gemm_choose(g, true));
    TRY(launch_gemm<bf16>(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_groupnorm(const mrisr_tensor* x, const mrisr_tensor* x2, const float* gamma_dev, const float* beta_dev,
                       int groups, float eps, int silu, mrisr_tensor* y, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    MRISR_REQUIRE(x->layout == MRISR_NHWC && y && y->dtype == x->dtype, "NHWC in/out, same dtype");
    hipStream_t st = (hipStream_t)stream;
    GroupNormArgs a;
    a.x0 = x->data; a.c0 = (int)x->shape[1];
    if (x2) { a.x1 = x2->data; a.c1 = (int)x2->shape[1]; }
    a.B = (int)x->shape[0]; a.HW = (int)(x->shape[2] * x->shape[3]); a.groups = groups; a.eps = eps;
    a.gamma = gamma_dev; a.beta = beta_dev; a.silu = silu; a.y = y->data;
    a.nsplit = groupnorm_nsplit(a.B, a.HW);
    DevBuf part;
    TRY(part.reserve((size_t)a.B * a.nsplit * groups * 2 * sizeof(float), false));
    a.partial = static_cast<float*>(part.p);
    int rc = x->dtype == MRISR_F32 ? launch_groupnorm<float>(a, st) : launch_groupnorm<bf16>(a, st);
    if (rc) return rc;
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_layernorm(const mrisr_tensor* x, const float* gamma_dev, const float* beta_dev, float eps,
                       mrisr_tensor* y, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    MRISR_REQUIRE(x->ndim == 2 && y && y->dtype == x->dtype, "rows in/out");
    hipStream_t st = (hipStream_t)stream;
    const int M = (int)x->shape[0], C = (int)x->shape[1];
    return x->dtype == MRISR_F32 ? launch_layernorm<float>(x->data, y->data, gamma_dev, beta_dev, M, C, eps, st)
                                 : launch_layernorm<bf16>(x->data, y->data, gamma_dev, beta_dev, M, C, eps, st);
    API_END
}

int mrisr_op_attention(const mrisr_tensor* q, const mrisr_tensor* k, const mrisr_tensor* v, int heads, int flash,
                       mrisr_tensor* out, void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(q));
    TRY(gemm_prepare());
    MRISR_REQUIRE(q->ndim == 3 && k && v && out && k->dtype == q->dtype && v->dtype == q->dtype && out->dtype == q->dtype,
                  "q,k,v,out: [B,N,C] same dtype");
    return q->dtype == MRISR_F32 ? op_attention_t<float>(q, k, v, heads, flash, out, (hipStream_t)stream)
                                 : op_attention_t<bf16>(q, k, v, heads, flash, out, (hipStream_t)stream);
    API_END
}

}  // extern "C"

// flash attention forward (with log-sum-exp) + backward on bf16 token rows: the kernels the fine-tuning step runs
static int op_attention_bwd_bf16(const mrisr_tensor* q, const mrisr_tensor* k, const mrisr_tensor* v, const mrisr_tensor* dout, int H,
                                 mrisr_tensor* dq, mrisr_tensor* dk, mrisr_tensor* dv, hipStream_t st) {
    typedef bf16 T;
    const int B = (int)q->shape[0], N = (int)q->shape[1], C = (int)q->shape[2], Nk = (int)k->shape[1];
    const int hd = C / H, BH = B * H;
    const int dpad = round_up(hd, 32), npad = round_up(N, 64), nkpad = round_up(Nk, 64);
    const size_t qsz = (size_t)BH * npad * dpad * sizeof(T), ksz = (size_t)BH * nkpad * dpad * sizeof(T);
    DevBuf qb, kb, vtb, vb, ktb, qtb, doh, doht, ob, lse, dsum;
    TRY(qb.reserve(qsz, true)); TRY(kb.reserve(ksz, true)); TRY(vtb.reserve(ksz, true)); TRY(vb.reserve(ksz, true));
    TRY(ktb.reserve(ksz, true)); TRY(qtb.reserve(qsz, true)); TRY(doh.reserve(qsz, true)); TRY(doht.reserve(qsz, true));
    TRY(ob.reserve((size_t)B * N * C * sizeof(T), false));
    TRY(lse.reserve((size_t)BH * npad * sizeof(float), true)); TRY(dsum.reserve((size_t)BH * npad * sizeof(float), true));
    auto conv = [&](const mrisr_tensor* x, void* dst, int n, int np, int tr) {
        hipLaunchKernelGGL(rows_to_heads_kernel<T>, dim3(1024), dim3(256), 0, st, static_cast<const T*>(x->data), static_cast<T*>(dst), B,
                           n, H, hd, np, dpad, tr);
    };
    conv(q, qb.p, N, npad, 0);
    conv(k, kb.p, Nk, nkpad, 0);
    conv(v, vtb.p, Nk, nkpad, 1);
    MRISR_CHECK_HIP(hipGetLastError());
    const float scale = 1.0f / sqrtf((float)hd);
    AttnArgs a;
    a.q = qb.p; a.k = kb.p; a.vt = vtb.p; a.out = ob.p;
    a.B = B; a.H = H; a.nq = N; a.nk = Nk; a.nkpad = nkpad; a.hd = hd; a.dpad = dpad; a.scale = scale;
    a.lse = static_cast<float*>(lse.p);
    TRY(launch_attention_bf16(a, st));
    TRY(launch_attention_bwd_prep(dout->data, ob.p, doh.p, static_cast<float*>(dsum.p), B, N, H, hd, npad, dpad, st));
    TRY(launch_transpose<T>(vtb.p, vb.p, dpad, nkpad, nkpad, dpad, (long long)dpad * nkpad, (long long)nkpad * dpad, BH, dpad, st));
    TRY(launch_transpose<T>(kb.p, ktb.p, nkpad, dpad, dpad, nkpad, (long long)nkpad * dpad, (long long)dpad * nkpad, BH, nkpad, st));
    TRY(launch_transpose<T>(qb.p, qtb.p, npad, dpad, dpad, npad, (long long)npad * dpad, (long long)dpad * npad, BH, npad, st));
    TRY(launch_transpose<T>(doh.p, doht.p, npad, dpad, dpad, npad, (long long)npad * dpad, (long long)dpad * npad, BH, npad, st));
    AttnBwdArgs g;
    g.q = qb.p; g.k = kb.p; g.v = vb.p; g.doh = doh.p; g.qt = qtb.p; g.kt = ktb.p; g.doht = doht.p;
    g.lse = static_cast<const float*>(lse.p); g.dsum = static_cast<const float*>(dsum.p);
    g.dq = dq->data; g.ldq = C; g.dk = dk->data; g.dv = dv->data; g.ldkv = C;
    g.B = B; g.H = H; g.nq = N; g.nk = Nk; g.npad = npad; g.nkpad = nkpad; g.hd = hd; g.dpad = dpad; g.scale = scale;
    TRY(launch_attention_bwd_bf16(g, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int mrisr_op_attention_bwd(const mrisr_tensor* q, const mrisr_tensor* k, const mrisr_tensor* v, const mrisr_tensor* dout,
                                      int heads, mrisr_tensor* dq, mrisr_tensor* dk, mrisr_tensor* dv, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(q && k && v && dout && dq && dk && dv && q->ndim == 3 && q->dtype == MRISR_BF16 && k->dtype == MRISR_BF16 &&
                      v->dtype == MRISR_BF16 && dout->dtype == MRISR_BF16 && dq->dtype == MRISR_BF16 && dk->dtype == MRISR_BF16 &&
                      dv->dtype == MRISR_BF16,
                  "attention backward: bf16 [B,N,C] tensors");
    MRISR_REQUIRE(heads >= 1 && q->shape[2] % heads == 0 && (q->shape[2] / heads) % 4 == 0, "head dim must be a multiple of 4");
    return op_attention_bwd_bf16(q, k, v, dout, heads, dq, dk, dv, (hipStream_t)stream);
    API_END
}

// =================================================================================================
// single-op entry points of the backward (tests/test_gpu_bwd_ops.py): the launchers of bwd.hip and the two composites of train_ops.h on
// the caller's device pointers.  Every argument the kernels index or vector-load by is checked before the first launch.
// =================================================================================================
namespace {
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int bwd_dtype_ok(int dtype) {
    MRISR_REQUIRE(dtype == MRISR_F32 || dtype == MRISR_BF16, "backward ops: f32 or bf16 operands");
    return 0;
}
template <typename T>
int op_groupnorm_bwd_t(const void* x0, int c0, const void* x1, int c1, int B, int HW, const float* gamma, const float* beta, int groups,
                       float eps, int silu, const void* dy, void* dx0, int acc0, void* dx1, int acc1, float* g_gamma, float* g_beta,
                       hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    const int C = c0 + c1;
    MRISR_REQUIRE(c0 % VE == 0 && c1 % VE == 0, "GroupNorm backward: channel counts in whole 16-byte vectors");
    MRISR_REQUIRE(al16(x0) && al16(x1) && al16(dy) && al16(dx0) && al16(dx1), "GroupNorm backward: 16-byte aligned operands");
    {
        const int nvec = C / VE;
        int vpt = 1;
        while (nvec / vpt > 256 || (nvec % vpt) != 0) ++vpt;
        MRISR_REQUIRE(vpt <= 4, "GroupNorm backward: too many channels");
    }
    OpScratch sc;
    GroupNormArgs f;
    f.x0 = x0; f.c0 = c0; f.x1 = x1; f.c1 = c1; f.B = B; f.HW = HW; f.groups = groups; f.eps = eps;
    f.gamma = gamma; f.beta = beta; f.silu = silu;
    f.nsplit = groupnorm_nsplit(B, HW);
    const size_t pbytes = (size_t)B * f.nsplit * groups * 2 * sizeof(float);
    f.y = sc.alloc((size_t)B * HW * C * sizeof(T));
    f.partial = static_cast<float*>(sc.alloc(pbytes));
    GroupNormBwdArgs a;
    a.x0 = x0; a.c0 = c0; a.x1 = x1; a.c1 = c1; a.B = B; a.HW = HW; a.groups = groups; a.eps = eps;
    a.gamma = gamma; a.beta = beta; a.silu = silu;
    a.dy = dy; a.dx0 = dx0; a.dx1 = dx1; a.acc0 = acc0 ? 1 : 0; a.acc1 = acc1 ? 1 : 0;
    a.fwd_partial = f.partial; a.nsplit = f.nsplit;
    a.bwd_partial = static_cast<float*>(sc.alloc(pbytes));
    if (!f.y || !f.partial || !a.bwd_partial) return 7;
    TRY(launch_groupnorm<T>(f, st));  // the forward statistics, exactly as the recorded forward leaves them
    TRY(launch_groupnorm_bwd<T>(a, st));
    if (g_gamma) TRY(launch_gn_affine_grad<T>(x0, dy, gamma, beta, f.partial, f.nsplit, groups, B, HW, C, eps, silu ? 1 : 0, g_gamma, g_beta, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
int op_lora_wgrad_t(const void* P, int ldp, const float* Q, int ldq, int M, int C, int mode, int r, int nmod, int secN, float* const out[3],
                    float scale, int geglu_half, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    MRISR_REQUIRE(C % VE == 0 && ldp % VE == 0 && ldp >= C && al16(P), "LoRA wgrad: P rows in whole, aligned 16-byte vectors");
    MRISR_REQUIRE(mode == 1 || (secN % VE == 0 && C == nmod * secN), "LoRA wgrad (dB): C = nmod sections of whole vectors");
    const int R = nmod * r, nq = (mode == 0 || R > 16) ? r : R;
    {   // the LDS tile of the kernel's geometry (lora_wgrad_geom)
        const int cx = C / VE, gx = (cx + 255) / 256, cxb = (cx + gx - 1) / gx, RL = 256 / cxb;
        MRISR_REQUIRE(RL <= 1 || (size_t)cxb * VE * nq * sizeof(float) <= 65536, "LoRA wgrad: LDS tile");
    }
    OpScratch sc;
    float* scratch = static_cast<float*>(sc.alloc(lora_wgrad_scratch_bytes(M, C, R, sizeof(T))));
    if (!scratch) return 7;
    TRY(launch_lora_wgrad<T>(P, ldp, Q, ldq, M, C, mode, r, nmod, secN, out, scale, scratch, st, geglu_half));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
int op_lora_wgrad_hr_t(const void* P, int ldp, const void* Q, int ldq, int M, int C, int mode, int r, int nmod, int secN, float* const out[3],
                       float scale, int geglu_half, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    MRISR_REQUIRE(ldp % VE == 0 && ldq % VE == 0 && ldq >= nmod * lora_hr_rp(r, (int)sizeof(T)),
                  "LoRA wgrad (high rank): rows in whole 16-byte vectors, Q rows of nmod * rp columns (rp: the rank rounded up to the K tile)");
    OpScratch sc;
    float* scratch = static_cast<float*>(sc.alloc(lora_wgrad_hr_scratch_bytes(M, C, mode, r, nmod, secN, sizeof(T))));
    if (!scratch) return 7;
    TRY(launch_lora_wgrad_hr<T>(P, ldp, Q, ldq, M, C, mode, r, nmod, secN, out, scale, scratch, st, geglu_half));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
int op_dora_scale_t(const float* W, const float* A, const float* B, const float* mag, float s, float* g, void* out, int ld, int n, int k, int r,
                    int geglu_half, int merged, hipStream_t st) {
    TRY(launch_dora_scale<T>(W, A, B, mag, s, g, out, ld, 0, n, k, r, geglu_half, merged, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
int op_dora_mag_grad_t(const void* P, int ldp, const void* Y, int ldy, const void* R, int ldr, const float* bias, const float* mag, float* gm, int M,
                       int C, int geglu_half, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    MRISR_REQUIRE(ldp % VE == 0 && ldy % VE == 0 && (!R || ldr % VE == 0), "DoRA magnitude gradient: row pitches in whole 16-byte vectors");
    OpScratch sc;
    float* scratch = static_cast<float*>(sc.alloc(dora_mag_grad_scratch_bytes(M, C, sizeof(T))));
    if (!scratch) return 7;
    TRY(launch_dora_mag_grad<T>(P, ldp, Y, ldy, R, ldr, bias, mag, gm, M, C, geglu_half, scratch, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
int op_conv_wgrad_t(const void* x, int xB, int xH, int xW, int cin_src, const void* dY, int ldy, int col0, int cout_src, int ks, int stride,
                    float* gW, float* gB, int cout, int cin, int geglu_half, hipStream_t st) {
    OpScratch sc;
    const int Ho = (xH - 1) / stride + 1, Wo = (xW - 1) / stride + 1;
    TRY(conv_wgrad_run<T>(st, false, [&](size_t n) { return sc.alloc(n); }, [&](GemmArgs& g) { return op_gemm_run<T>(sc, st, g); }, x, xB, xH,
                          xW, cin_src, dY, ldy, col0, Ho, Wo, cout_src, ks, stride, gW, gB, cout, cin, geglu_half));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
int op_conv_dgrad_t(const void* dy, int B, int H, int W, int cout, const float* w, int cin, int mode, void* dx, int accumulate,
                    hipStream_t st) {
    OpScratch sc;
    void* wd = sc.alloc((size_t)cout * cin * 9 * sizeof(T));
    if (!wd) return 7;
    TRY(launch_pack_conv_dgrad<T>(w, wd, cout, cin, st));  // the packer of train_prepare
    TRY(conv_dgrad_run<T>(st, false, [&](GemmArgs& g) { return op_gemm_run<T>(sc, st, g); }, dy, B, H, W, cout, cin, wd, mode, dx,
                          accumulate ? dx : nullptr, cin));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}
}  // namespace

#define BWD_DISPATCH(dtype, fn, ...) ((dtype) == MRISR_F32 ? fn<float>(__VA_ARGS__) : fn<bf16>(__VA_ARGS__))

extern "C" {

int mrisr_op_groupnorm_bwd(int dtype, const void* x0, int c0, const void* x1, int c1, int B, int HW, const float* gamma_dev,
                           const float* beta_dev, int groups, float eps, int silu, const void* dy, void* dx0, int acc0, void* dx1,
                           int acc1, float* g_gamma, float* g_beta, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(x0 && gamma_dev && beta_dev && dy && dx0 && B >= 1 && HW >= 1 && c0 >= 1 && c1 >= 0, "GroupNorm backward: null / empty operand");
    MRISR_REQUIRE((c1 > 0) == (x1 != nullptr) && (c1 > 0) == (dx1 != nullptr), "GroupNorm backward: x1 / dx1 exactly when c1 > 0");
    MRISR_REQUIRE(groups >= 1 && groups <= 64 && (c0 + c1) % groups == 0, "GroupNorm backward: at most 64 groups dividing the channels");
    MRISR_REQUIRE((g_gamma != nullptr) == (g_beta != nullptr) && (!g_gamma || c1 == 0), "GroupNorm affine gradients: both, on a single source");
    return BWD_DISPATCH(dtype, op_groupnorm_bwd_t, x0, c0, x1, c1, B, HW, gamma_dev, beta_dev, groups, eps, silu, dy, dx0, acc0, dx1, acc1,
                        g_gamma, g_beta, (hipStream_t)stream);
    API_END
}

int mrisr_op_layernorm_bwd(int dtype, const void* x, const void* dy, void* dx, const float* gamma_dev, int M, int C, float eps,
                           int accumulate, float* g_gamma, float* g_beta, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    const int VE = dtype == MRISR_F32 ? 4 : 8;
    MRISR_REQUIRE(x && dy && (dx || g_gamma) && M >= 1 && C >= 1, "LayerNorm backward: null / empty operand");
    MRISR_REQUIRE(!dx || (gamma_dev && C % VE == 0 && C / VE <= 5 * 64 && al16(x) && al16(dy) && al16(dx)),
                  "LayerNorm backward: rows of at most 320 aligned 16-byte vectors");
    MRISR_REQUIRE((g_gamma != nullptr) == (g_beta != nullptr) && (!g_gamma || C <= 64 * 24), "LayerNorm affine gradients: both, C <= 1536");
    if (dx) TRY(BWD_DISPATCH(dtype, launch_layernorm_bwd, x, dy, dx, gamma_dev, M, C, eps, accumulate ? 1 : 0, st));
    if (g_gamma) TRY(BWD_DISPATCH(dtype, launch_ln_affine_grad, x, dy, M, C, eps, g_gamma, g_beta, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_geglu(int dtype, int backward, const void* pre, const void* dout, void* out, int64_t M, int half, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(pre && out && (!backward || dout) && M >= 1 && half >= 16, "GEGLU: null / empty operand");
    MRISR_REQUIRE(half % 16 == 0, "GEGLU: the (value, gate) interleave is 16 columns wide");
    if (backward) TRY(BWD_DISPATCH(dtype, launch_geglu_bwd, pre, dout, out, (long long)M, half, st));
    else TRY(BWD_DISPATCH(dtype, launch_geglu_fwd, pre, out, (long long)M, half, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_pointwise_bwd(int kind, int dtype, const void* a, const void* b, void* out, float* out_f32, int64_t n, int B, int H, int W,
                           int C, int flag, int ld_out, int off, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(kind >= 0 && kind <= 5 && a, "pointwise backward: kind 0..5, operand a");
    if (kind <= 1) {
        MRISR_REQUIRE(b && out && n >= 1, "silu_bwd / relu_bwd: b, out, n elements");
        if (kind == 0) TRY(BWD_DISPATCH(dtype, launch_silu_bwd, a, b, out, (long long)n, st));
        else TRY(BWD_DISPATCH(dtype, launch_relu_bwd, a, b, out, (long long)n, st));
    } else {
        MRISR_REQUIRE(B >= 1 && H >= 1 && W >= 1 && C >= 1 && (long long)B * H * W * C < (1ll << 31), "pointwise backward: [B][H][W][C] extents");
        if (kind == 2) {
            MRISR_REQUIRE(out, "sumpool2: out");
            TRY(BWD_DISPATCH(dtype, launch_sumpool2, a, out, B, H, W, C, flag ? 1 : 0, st));
        } else if (kind == 3) {
            MRISR_REQUIRE(b && out && out_f32, "mse_grad: target, d pred, loss");
            MRISR_CHECK_HIP(hipMemsetAsync(out_f32, 0, sizeof(float), st));
            TRY(BWD_DISPATCH(dtype, launch_mse_grad, a, static_cast<const float*>(b), out, out_f32, B, C, H, W, st));
        } else if (kind == 4) {
            MRISR_REQUIRE(out_f32 && off >= 0 && off + C <= ld_out, "rowvec_grad: columns off .. off + C inside the row pitch");
            TRY(BWD_DISPATCH(dtype, launch_rowvec_grad, a, out_f32, ld_out, off, B, H * W, C, flag ? 1 : 0, st));
        } else {
            MRISR_REQUIRE(out_f32, "colsum: out");
            TRY(BWD_DISPATCH(dtype, launch_colsum_gen, a, C, 0, out_f32, B * H * W, C, 0, st));
        }
    }
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_lora_wgrad(int dtype, const void* P, int ldp, const float* Q, int ldq, int M, int C, int mode, int r, int nmod, int secN,
                        float* out0, float* out1, float* out2, float scale, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(P && Q && M >= 1 && C >= 1 && (mode == 0 || mode == 1), "LoRA wgrad: null / empty operand, mode 0 / 1");
    MRISR_REQUIRE(r % 4 == 0 && r >= 4 && r <= 16 && nmod >= 1 && nmod <= 3, "LoRA wgrad: rank 4/8/12/16, <= 3 fused modules");
    MRISR_REQUIRE(ldq % 4 == 0 && ldq >= nmod * r && al16(Q), "LoRA wgrad: Q rows in whole, aligned 16-byte vectors");
    float* const out[3] = {out0, nmod > 1 ? out1 : nullptr, nmod > 2 ? out2 : nullptr};
    return BWD_DISPATCH(dtype, op_lora_wgrad_t, P, ldp, Q, ldq, M, C, mode, r, nmod, secN, out, scale, 0, (hipStream_t)stream);
    API_END
}

int mrisr_op_lora_wgrad_geglu(int dtype, const void* P, int ldp, const float* Q, int ldq, int M, int half, int r, float* out, float scale,
                              void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(P && Q && out && M >= 1 && half >= 16 && half <= (1 << 20), "LoRA wgrad (GEGLU): null / empty operand");
    MRISR_REQUIRE(half % 16 == 0, "LoRA wgrad (GEGLU): the (value, gate) interleave is 16 columns wide");
    MRISR_REQUIRE(r % 4 == 0 && r >= 4 && r <= 16, "LoRA wgrad: rank 4/8/12/16");
    MRISR_REQUIRE(ldq % 4 == 0 && ldq >= r && al16(Q), "LoRA wgrad: Q rows in whole, aligned 16-byte vectors");
    float* const o[3] = {out, nullptr, nullptr};
    return BWD_DISPATCH(dtype, op_lora_wgrad_t, P, ldp, Q, ldq, M, 2 * half, 0, r, 1, 2 * half, o, scale, half, (hipStream_t)stream);
    API_END
}

int mrisr_op_lora_wgrad_hr(int dtype, const void* P, int ldp, const void* Q, int ldq, int M, int C, int mode, int r, int nmod, int secN,
                           float* out0, float* out1, float* out2, float scale, int geglu_half, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(P && Q && M >= 1 && C >= 1 && (mode == 0 || mode == 1), "LoRA wgrad (high rank): null / empty operand, mode 0 / 1");
    MRISR_REQUIRE(lora_rank_high(r) && nmod >= 1 && nmod <= 3, "LoRA wgrad (high rank): rank 32 .. 128 in steps of 16, <= 3 fused modules");
    MRISR_REQUIRE(C % 8 == 0 && ldp >= C && al16(P) && al16(Q), "LoRA wgrad (high rank): C a multiple of 8, P rows of at least C, 16-byte aligned operands");
    MRISR_REQUIRE(mode == 1 || (secN >= 8 && secN % 8 == 0 && C == nmod * secN), "LoRA wgrad (high rank, dB): C = nmod sections of whole vectors");
    MRISR_REQUIRE(geglu_half == 0 || (mode == 0 && nmod == 1 && geglu_half % 16 == 0 && C == 2 * geglu_half),
                  "LoRA wgrad (high rank): the GEGLU interleave is for dB of one [2 * half] projection, half a multiple of 16");
    float* const out[3] = {out0, nmod > 1 ? out1 : nullptr, nmod > 2 ? out2 : nullptr};
    MRISR_REQUIRE(!geglu_half || out0, "LoRA wgrad (high rank, GEGLU): out");
    return BWD_DISPATCH(dtype, op_lora_wgrad_hr_t, P, ldp, Q, ldq, M, C, mode, r, nmod, secN, out, scale, geglu_half, (hipStream_t)stream);
    API_END
}

int mrisr_op_dora_scale(int dtype, const float* W, const float* A, const float* B, const float* mag, float scale, float* g, void* out, int ld,
                        int n, int k, int r, int geglu_half, int merged, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(W && A && B && mag && g && out && n >= 1 && k >= 1, "DoRA scale: null / empty operand");
    MRISR_REQUIRE(al16(W) && al16(A) && al16(B) && al16(mag) && al16(g) && al16(out), "DoRA scale: 16-byte aligned operands");
    MRISR_REQUIRE(lora_rank_low(r) || lora_rank_high(r), "DoRA scale: rank 4 / 8 / 12 / 16 or 32 .. 128 in steps of 16");
    MRISR_REQUIRE(ld >= k, "DoRA scale: the output pitch covers a row");
    MRISR_REQUIRE(geglu_half == 0 || (geglu_half % 16 == 0 && n == 2 * geglu_half), "DoRA scale: the GEGLU interleave is for n = 2 * half rows, half a multiple of 16");
    return BWD_DISPATCH(dtype, op_dora_scale_t, W, A, B, mag, scale, g, out, ld, n, k, r, geglu_half, merged ? 1 : 0, (hipStream_t)stream);
    API_END
}

int mrisr_op_dora_mag_grad(int dtype, const void* P, int ldp, const void* Y, int ldy, const void* R, int ldr, const float* bias, const float* mag,
                           float* gm, int M, int C, int geglu_half, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(P && Y && mag && gm && M >= 1 && C >= 1, "DoRA magnitude gradient: null / empty operand");
    MRISR_REQUIRE(C % 8 == 0 && ldp >= C && ldy >= C && (!R || ldr >= C), "DoRA magnitude gradient: C a multiple of 8, rows of at least C");
    MRISR_REQUIRE(al16(P) && al16(Y) && al16(R) && al16(bias) && al16(mag) && al16(gm), "DoRA magnitude gradient: 16-byte aligned operands");
    MRISR_REQUIRE(geglu_half == 0 || (geglu_half % 16 == 0 && C == 2 * geglu_half), "DoRA magnitude gradient: the GEGLU interleave is for C = 2 * half, half a multiple of 16");
    return BWD_DISPATCH(dtype, op_dora_mag_grad_t, P, ldp, Y, ldy, R, ldr, bias, mag, gm, M, C, geglu_half, (hipStream_t)stream);
    API_END
}

int mrisr_op_transpose(int dtype, const void* src, void* dst, int R, int C, int ld_src, int ld_dst, int64_t bs_src, int64_t bs_dst,
                       int batch, int r_valid, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(src && dst && R >= 1 && C >= 1 && batch >= 1 && batch <= 65535, "transpose: null / empty operand");
    MRISR_REQUIRE(ld_src >= C && ld_dst >= R && r_valid >= 0 && r_valid <= R, "transpose: pitches cover the rows, r_valid <= R");
    MRISR_REQUIRE(batch == 1 || (bs_src >= (long long)(R - 1) * ld_src + C && bs_dst >= (long long)(C - 1) * ld_dst + R),
                  "transpose: batch strides cover one matrix");
    TRY(BWD_DISPATCH(dtype, launch_transpose, src, dst, R, C, ld_src, ld_dst, (long long)bs_src, (long long)bs_dst, batch, r_valid, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_attn_identity(int dtype, const void* vt, void* out, int B, int H, int N, int hd, int npad, int dpad, int first_sample, int n_samples,
                           void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    // (the launcher refuses null / misaligned pointers, npad < N, dpad < hd and a range outside B before it launches)
    TRY(BWD_DISPATCH(dtype, launch_attn_identity, vt, out, B, H, N, hd, npad, dpad, first_sample, n_samples, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_freeu(int dtype, const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs, float b,
                   float s, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    // (the launcher refuses null / misaligned pointers, an empty geometry, Ch % 16, Cs % 8 and bad scalars before it launches)
    TRY(BWD_DISPATCH(dtype, launch_freeu, hidden, skip, hidden_out, skip_out, B, H, W, Ch, Cs, b, s, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// one FreeU stage with (b, s) of up block `stage` read by the kernel from row `slot` of a host schedule table (uploaded here)
int mrisr_op_freeu_scheduled(int dtype, const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W, int Ch, int Cs,
                             int stage, const float* sched_host, int n_rows, int slot, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(stage == 0 || stage == 1, "freeu: stage 0 (s1, b1) or 1 (s2, b2)");
    MRISR_REQUIRE(sched_host && n_rows >= 1 && n_rows <= 65536, "freeu: a schedule table of 1 .. 65536 rows");
    MRISR_REQUIRE(slot >= 0 && slot < n_rows, "freeu: slot outside the schedule table");
    TRY(check_schedule_rows(sched_host, n_rows));
    DevBuf d_sched, d_step;
    TRY(d_sched.reserve(sizeof(float) * 8 * (size_t)n_rows, false));
    TRY(d_step.reserve(16, true));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_sched.p, sched_host, sizeof(float) * 8 * (size_t)n_rows, hipMemcpyHostToDevice, st));
    MRISR_CHECK_HIP(hipMemcpyAsync(d_step.p, &slot, sizeof(int), hipMemcpyHostToDevice, st));
    TRY(BWD_DISPATCH(dtype, launch_freeu_sched, hidden, skip, hidden_out, skip_out, B, H, W, Ch, Cs, static_cast<const float*>(d_sched.p),
                     static_cast<const int*>(d_step.p), 5 + stage, 3 + stage, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// the multi-tensor scaled add of the conditioning table alone (condctl.hip): x_k += w_k * table[slot][col] * r_k on rows [row_lo, row_hi) of
// x_k, for n_pairs pairs in one launch; table_host NULL: the factor is w_k
int mrisr_op_cond_add(int dtype, int n_pairs, void* const* x, const void* const* r, const int64_t* per_row, const float* weights,
                      const float* table_host, int n_rows, int slot, int col, int row_lo, int row_hi, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(dtype == MRISR_F32 || dtype == MRISR_BF16, "cond add: f32 or bf16 operands");
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(x && r && per_row && weights && n_pairs >= 1 && n_pairs <= COND_MAX_PAIRS, "cond add: 1 .. 16 pairs with their weights");
    CondAddArgs a{};
    DevBuf d_table, d_step;
    if (table_host) {
        MRISR_REQUIRE(n_rows >= 1 && n_rows <= 65536 && slot >= 0 && slot < n_rows, "cond add: a table of 1 .. 65536 rows, slot inside it");
        MRISR_REQUIRE(col == 0 || col == 1, "cond add: column 0 (c) or 1 (a)");
        TRY(check_conditioning_rows(table_host, n_rows));
        TRY(d_table.reserve(sizeof(float) * 4 * (size_t)n_rows, false));
        TRY(d_step.reserve(16, true));
        MRISR_CHECK_HIP(hipMemcpyAsync(d_table.p, table_host, sizeof(float) * 4 * (size_t)n_rows, hipMemcpyHostToDevice, st));
        MRISR_CHECK_HIP(hipMemcpyAsync(d_step.p, &slot, sizeof(int), hipMemcpyHostToDevice, st));
        a.table = static_cast<const float*>(d_table.p); a.step = static_cast<const int*>(d_step.p); a.col = col;
    }
    a.n_pairs = n_pairs; a.row_lo = row_lo; a.row_hi = row_hi;
    for (int k = 0; k < n_pairs; ++k) { a.pair[k].x = x[k]; a.pair[k].r = r[k]; a.pair[k].per = per_row[k]; a.pair[k].w = weights[k]; }
    // (the launcher refuses null / misaligned pointers, empty pairs, an empty row range and weights that are not finite before it launches)
    TRY(BWD_DISPATCH(dtype, launch_cond_add, a, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

// the consistency launch alone (consist.hip): table and step counter already on the device
int mrisr_op_consistency(float* x, float* xK, int K, const float* ref, const float* lr, const float* noise, const float* table_dev,
                         const int* step_dev, int B, int C, int h, int w, int factor, int filter, void* stream) {
    API_BEGIN
    hipStream_t st = (hipStream_t)stream;
    ConsistArgs a;
    a.x = x; a.xK = xK; a.K = K; a.ref = ref; a.lr = lr; a.noise = noise; a.table = table_dev; a.step = step_dev;
    a.B = B; a.C = C; a.h = h; a.w = w; a.factor = factor; a.filter = filter;
    // (the launcher refuses null / misaligned pointers, K, the factor, the filter and the LDS need before it launches)
    TRY(launch_consistency(a, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_softmax_bwd(int dtype, const void* p, const float* dp, void* ds, int ld, int64_t rows, int nk, float scale, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(p && dp && ds && rows >= 1 && nk >= 1 && nk <= ld, "softmax backward: null / empty operand, nk <= ld");
    MRISR_REQUIRE(ld % 4 != 0 || ld > 4096 || (al16(p) && al16(dp) && al16(ds)), "softmax backward: aligned rows for the vector kernel");
    TRY(BWD_DISPATCH(dtype, launch_softmax_bwd, p, dp, ds, ld, (long long)rows, nk, scale, st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_small_dense_bwd(int dtype, int which, const float* dY, int ldy, const void* xw, int ldx, int rows, int N, int K, int silu_in,
                             const float* pre, int ldpre, float* out, float* gB, int ld_out, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    hipStream_t st = (hipStream_t)stream;
    MRISR_REQUIRE(dY && xw && out && (which == 0 || which == 1), "small dense backward: null operand, which 0 / 1");
    MRISR_REQUIRE(rows >= 1 && rows <= 64 && N >= 1 && K >= 1 && ldy >= N, "small dense backward: 1..64 rows, dY pitch covers N");
    if (which == 0) {
        MRISR_REQUIRE(ldx >= K, "small wgrad: X pitch covers K");
        TRY(launch_small_wgrad(dY, ldy, static_cast<const float*>(xw), ldx, rows, N, K, silu_in ? 1 : 0, out, gB, st));
    } else {
        MRISR_REQUIRE(ld_out >= K && (!pre || ldpre >= K), "small dgrad: dX / pre pitches cover K");
        TRY(BWD_DISPATCH(dtype, launch_small_dgrad, dY, ldy, xw, rows, N, K, pre, ldpre, out, ld_out, st));
    }
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

int mrisr_op_conv_wgrad(int dtype, const void* x, int xB, int xH, int xW, int cin_src, const void* dY, int ldy, int col0, int cout_src,
                        int ks, int stride, float* gW, float* gB, int cout, int cin, int geglu_half, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    TRY(gemm_prepare());
    MRISR_REQUIRE(x && dY && gW && xB >= 1 && xH >= 1 && xW >= 1, "conv wgrad: null / empty operand");
    MRISR_REQUIRE((ks == 1 || ks == 3) && (stride == 1 || stride == 2), "conv wgrad: 1x1 or 3x3, stride 1 or 2");
    MRISR_REQUIRE(cout >= 1 && cout <= cout_src && cin >= 1 && cin <= cin_src, "conv wgrad: raw tensor inside the (padded) layer");
    MRISR_REQUIRE(col0 >= 0 && col0 + cout_src <= ldy, "conv wgrad: dY columns inside the row pitch");
    MRISR_REQUIRE(geglu_half == 0 || (geglu_half % 16 == 0 && cout == 2 * geglu_half), "conv wgrad: GEGLU interleave of a [2 * half] projection");
    MRISR_REQUIRE((long long)xB * xH * xW < (1ll << 24) && (long long)ks * ks * cin_src * cout_src < (1ll << 28), "conv wgrad: extents");
    return BWD_DISPATCH(dtype, op_conv_wgrad_t, x, xB, xH, xW, cin_src, dY, ldy, col0, cout_src, ks, stride, gW, gB, cout, cin, geglu_half,
                        (hipStream_t)stream);
    API_END
}

int mrisr_op_conv_dgrad(int dtype, const void* dy, int B, int H, int W, int cout, const float* w_oihw_dev, int cin, int mode, void* dx,
                        int accumulate, void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    TRY(gemm_prepare());
    MRISR_REQUIRE(dy && w_oihw_dev && dx && B >= 1 && H >= 1 && W >= 1 && cout >= 1 && cin >= 1, "conv dgrad: null / empty operand");
    MRISR_REQUIRE(mode == 0 || mode == 1, "conv dgrad: mode 0 (stride 1) or 1 (stride 2)");
    const int bk = dtype == MRISR_F32 ? 32 : 64;
    MRISR_REQUIRE(mode == 0 || (cout % bk == 0 && cin % 4 == 0), "strided dgrad of a tiny conv");
    MRISR_REQUIRE(al16(dy) && al16(dx), "conv dgrad: 16-byte aligned activations");
    return BWD_DISPATCH(dtype, op_conv_dgrad_t, dy, B, H, W, cout, w_oihw_dev, cin, mode, dx, accumulate, (hipStream_t)stream);
    API_END
}

int mrisr_op_conv_lora_down(int dtype, const void* x_nhwc, int B, int H, int W, int cin, const float* a_dev, int r, float* z, int route,
                            void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(x_nhwc && a_dev && z && B >= 1 && H >= 1 && W >= 1, "conv_lora_down: null / empty operand");
    MRISR_REQUIRE(r >= 1 && r <= 16 && cin >= 1 && cin % (dtype == MRISR_F32 ? 4 : 8) == 0, "conv_lora_down: rank <= 16, channels in 16-byte pieces");
    MRISR_REQUIRE(al16(x_nhwc) && al16(z) && (long long)B * H * W * std::max(cin, 16) < (1ll << 31), "conv_lora_down: alignment / extents");
    return BWD_DISPATCH(dtype, op_conv_lora_down_t, x_nhwc, B, H, W, cin, a_dev, r, z, route, (hipStream_t)stream);
    API_END
}

int mrisr_op_conv_lora_dgrad(int dtype, const float* dz, int B, int H, int W, int r, const float* a_dev, int cin, void* dx_nhwc, int accumulate,
                             void* stream) {
    API_BEGIN
    TRY(bwd_dtype_ok(dtype));
    MRISR_REQUIRE(dz && a_dev && dx_nhwc && B >= 1 && H >= 1 && W >= 1, "conv_lora_dgrad: null / empty operand");
    MRISR_REQUIRE((r == 4 || r == 8 || r == 12 || r == 16) && cin >= 4 && cin % 4 == 0, "conv_lora_dgrad: rank 4 / 8 / 12 / 16, channels in fours");
    MRISR_REQUIRE(al16(dz) && al16(dx_nhwc) && (long long)B * H * W * cin < (1ll << 31), "conv_lora_dgrad: alignment / extents");
    return BWD_DISPATCH(dtype, op_conv_lora_dgrad_t, dz, B, H, W, r, a_dev, cin, dx_nhwc, accumulate, (hipStream_t)stream);
    API_END
}

int mrisr_op_conv3x3_lora(const mrisr_tensor* x, const float* w_oihw_dev, const float* bias_dev, const float* a_dev, const float* b_dev, int r,
                          float scale, const float* rowvec_dev, const mrisr_tensor* resid, int cout, int splitk, int tile, mrisr_tensor* y,
                          void* stream) {
    API_BEGIN
    TRY(op_dtype_ok(x));
    TRY(gemm_prepare());
    MRISR_REQUIRE(w_oihw_dev && y && (r == 0 || (a_dev && b_dev)), "conv3x3 + LoRA: null argument");
    MRISR_REQUIRE(x->layout == MRISR_NHWC && y->layout == MRISR_NHWC && y->dtype == x->dtype && (!resid || (resid->layout == MRISR_NHWC && resid->dtype == x->dtype)),
                  "NHWC in/out, same dtype");
    MRISR_REQUIRE(y->shape[0] == x->shape[0] && y->shape[1] == cout && y->shape[2] == x->shape[2] && y->shape[3] == x->shape[3], "conv output shape");
    MRISR_REQUIRE(!resid || (resid->shape[0] == y->shape[0] && resid->shape[1] == cout && resid->shape[2] == y->shape[2] && resid->shape[3] == y->shape[3]),
                  "residual of the output's shape");
    MRISR_REQUIRE(r >= 0 && r <= 16 && x->shape[1] % (x->dtype == MRISR_F32 ? 32 : 64) == 0 && cout % 4 == 0, "conv3x3 + LoRA: rank <= 16, whole K tiles");
    hipStream_t st = (hipStream_t)stream;
    return x->dtype == MRISR_F32 ? op_conv3x3_lora_t<float>(x, w_oihw_dev, bias_dev, a_dev, b_dev, r, scale, rowvec_dev, resid, cout, splitk, tile, y, st)
                                 : op_conv3x3_lora_t<bf16>(x, w_oihw_dev, bias_dev, a_dev, b_dev, r, scale, rowvec_dev, resid, cout, splitk, tile, y, st);
    API_END
}

// ---- tiled sampling: the gather and the blend alone, on explicit origin / weight arrays (uploaded to a scratch table for the call) ----
static int op_tile_plan(const mrisr_tensor* x, const mrisr_tensor* xt, const int* oy, int ky, const int* ox, int kx, const float* wy,
                        const float* wx, TilePlan* p) {
    MRISR_REQUIRE(x && xt && x->data && xt->data && oy && ox, "tile op: null argument");
    MRISR_REQUIRE(x->ndim == 4 && xt->ndim == 4 && x->dtype == MRISR_F32 && xt->dtype == MRISR_F32 && x->layout == MRISR_NCHW &&
                  xt->layout == MRISR_NCHW, "tile op: canvas and tile batch must be f32 NCHW [.., C, H, W]");
    MRISR_REQUIRE((reinterpret_cast<uintptr_t>(x->data) & 3) == 0 && (reinterpret_cast<uintptr_t>(xt->data) & 3) == 0, "tile op: misaligned pointer");
    for (int d = 0; d < 4; ++d)
        MRISR_REQUIRE(x->shape[d] > 0 && xt->shape[d] > 0 && x->shape[d] < (1ll << 31) && xt->shape[d] < (1ll << 31), "tile op: empty tensor");
    MRISR_REQUIRE(ky > 0 && kx > 0 && ky <= x->shape[2] && kx <= x->shape[3], "tile op: tile counts");
    MRISR_REQUIRE(xt->shape[0] == x->shape[0] * ky * kx && xt->shape[1] == x->shape[1],
                  "tile op: the tile batch must be [NB * ky * kx, C, tile_h, tile_w] for a canvas [NB, C, H, W]");
    p->H = (int)x->shape[2]; p->W = (int)x->shape[3]; p->th = (int)xt->shape[2]; p->tw = (int)xt->shape[3];
    p->oy.assign(oy, oy + ky);
    p->ox.assign(ox, ox + kx);
    if (wy && wx && p->th <= p->H && p->tw <= p->W) {
        p->nwy.assign(wy, wy + (size_t)ky * p->th);
        p->nwx.assign(wx, wx + (size_t)kx * p->tw);
    } else {  // the gather reads no weights
        p->nwy.assign((size_t)ky * p->th, 1.f);
        p->nwx.assign((size_t)kx * p->tw, 1.f);
    }
    TRY(p->check());
    p->pack();
    return 0;
}
int mrisr_op_tile_gather(const mrisr_tensor* x, mrisr_tensor* xt, const int* origins_y, int ky, const int* origins_x, int kx, void* stream) {
    API_BEGIN
    TilePlan p;
    TRY(op_tile_plan(x, xt, origins_y, ky, origins_x, kx, nullptr, nullptr, &p));
    hipStream_t st = (hipStream_t)stream;
    DevBuf tab;
    TRY(tab.reserve(p.bytes(), false));
    MRISR_CHECK_HIP(hipMemcpyAsync(tab.p, p.words.data(), p.bytes(), hipMemcpyHostToDevice, st));
    TRY(launch_tile_gather((const float*)x->data, (float*)xt->data, p.grid(tab.p), (int)x->shape[0], (int)x->shape[1], st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));  // the table is freed on return
    return 0;
    API_END
}
int mrisr_op_tile_blend(const mrisr_tensor* xt, mrisr_tensor* x, const int* origins_y, int ky, const int* origins_x, int kx,
                        const float* weights_y, const float* weights_x, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(weights_y && weights_x, "tile blend: null weight table");
    TilePlan p;
    TRY(op_tile_plan(x, xt, origins_y, ky, origins_x, kx, weights_y, weights_x, &p));
    hipStream_t st = (hipStream_t)stream;
    DevBuf tab;
    TRY(tab.reserve(p.bytes(), false));
    MRISR_CHECK_HIP(hipMemcpyAsync(tab.p, p.words.data(), p.bytes(), hipMemcpyHostToDevice, st));
    TRY(launch_tile_blend((const float*)xt->data, (float*)x->data, p.grid(tab.p), (int)x->shape[0], (int)x->shape[1], st));
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
    API_END
}

}  // extern "C"
#undef BWD_DISPATCH

// =================================================================================================
// GEMM micro-benchmark (tools/gemm_sweep.py): times one implicit-GEMM shape with a forced tile / split-K on
// pseudo-random operands (zero-filled operands would flatter the clock; guide rule 25).
// =================================================================================================
__global__ void fill_random_bf16_kernel(bf16* p, long long n, unsigned seed) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        unsigned x = (unsigned)i * 2654435761u + seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        p[i] = (bf16)(((float)(x & 0xFFFF) / 32768.0f - 1.0f) * 0.5f);
    }
}
extern "C" void mrisr_debug_force_tile(int t);
extern "C" int mrisr_bench_mlp(int M, int hidden, int iters, float* ms_out) {
    API_BEGIN
    TRY(gemm_prepare());
    hipStream_t st = nullptr;
    const int C = 320;
    DevBuf x, w1, w2, o, b1, b2, gb;
    TRY(x.reserve((size_t)M * C * 2, false));
    TRY(o.reserve((size_t)M * C * 2, false));
    TRY(w1.reserve((size_t)2 * hidden * C * 2, false));
    TRY(w2.reserve((size_t)C * hidden * 2, false));
    TRY(b1.reserve((size_t)2 * hidden * 4, true));
    TRY(b2.reserve((size_t)C * 4, true));
    TRY(gb.reserve((size_t)C * 4, true));
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(2048), dim3(256), 0, st, (bf16*)x.p, (long long)M * C, 1u);
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(2048), dim3(256), 0, st, (bf16*)w1.p, (long long)2 * hidden * C, 2u);
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(2048), dim3(256), 0, st, (bf16*)w2.p, (long long)C * hidden, 3u);
    MlpArgs a;
    a.x = x.p; a.ldx = C; a.M = M; a.ln_gamma = (const float*)gb.p; a.ln_beta = (const float*)gb.p;
    a.w1 = w1.p; a.b1 = (const float*)b1.p; a.w2p = w2.p; a.b2 = (const float*)b2.p;
    a.resid = x.p; a.ldr = C; a.out = o.p; a.ldo = C; a.C = C; a.H = hidden; a.N2 = C;
    for (int i = 0; i < 2; ++i) TRY(launch_mlp_fused(a, st));
    hipEvent_t e0, e1;
    MRISR_CHECK_HIP(hipEventCreate(&e0));
    MRISR_CHECK_HIP(hipEventCreate(&e1));
    MRISR_CHECK_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) (void)launch_mlp_fused(a, st);
    MRISR_CHECK_HIP(hipEventRecord(e1, st));
    MRISR_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    MRISR_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
    API_END
}

extern "C" int mrisr_bench_gemm(int M, int N, int K, int conv, int B, int H, int W, int stride, int ups, int c1,
                                int tile, int splitk, int iters, float* ms_out) {
    API_BEGIN
    TRY(gemm_prepare());
    hipStream_t st = nullptr;
    GemmArgs g;
    const int Cin = conv ? K / 9 : K;
    const int c0 = Cin - c1;
    DevBuf a0, a1, wb, ob, part, bias;
    const long long a_rows = conv ? (long long)B * H * W : M;
    TRY(a0.reserve((size_t)a_rows * c0 * 2, false));
    if (c1) TRY(a1.reserve((size_t)a_rows * c1 * 2, false));
    TRY(wb.reserve((size_t)N * K * 2, false));
    TRY(ob.reserve((size_t)M * N * 2, false));
    TRY(bias.reserve((size_t)N * 4, true));
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(2048), dim3(256), 0, st, (bf16*)a0.p, a_rows * c0, 1u);
    if (c1) hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(2048), dim3(256), 0, st, (bf16*)a1.p, a_rows * c1, 2u);
    hipLaunchKernelGGL(fill_random_bf16_kernel, dim3(2048), dim3(256), 0, st, (bf16*)wb.p, (long long)N * K, 3u);
    ga_rows(g, a0.p, c0, c0);
    if (c1) ga_rows2(g, a1.p, c1, c1);
    if (conv) {
        ga_conv3(g, B, H, W, stride, ups);
        MRISR_REQUIRE(M == B * g.Hout * g.Wout, "bench conv M");
    }
    ga_weight(g, wb.p, M, N, K); g.bias = (const float*)bias.p; ga_out(g, ob.p, N);
    if (const char* e = getenv("MRISR_BENCH_NOSTORE")) { if (e[0] == '1') g.out_mode = OUT_NONE; }  // experiment: epilogue without the store
    ForcedTile forced(tile);
    TRY(op_plan<bf16>(g, splitk, false, part));
    for (int i = 0; i < 2; ++i) TRY(launch_gemm<bf16>(g, st));
    hipEvent_t e0, e1;
    MRISR_CHECK_HIP(hipEventCreate(&e0));
    MRISR_CHECK_HIP(hipEventCreate(&e1));
    MRISR_CHECK_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) (void)launch_gemm<bf16>(g, st);
    MRISR_CHECK_HIP(hipEventRecord(e1, st));
    MRISR_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    MRISR_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return g.splitk * 1000 == 0 ? 0 : 0;
    API_END
}
