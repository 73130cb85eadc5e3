// Describing and running one GEMM launch from the host: the builders that fill the recurring field groups of
// GemmArgs, the one plan-allocate-launch path, and the attention core that Runner, Trainer and the single-op entry point share.
// Plain functions on the plain structs: a field no builder is called for keeps the struct's default.
#pragma once
#include <cmath>
#include <cstdint>

#include "api.h"
#include "runtime.h"

namespace mrisr {

// ---- A operand ----
inline void ga_rows(GemmArgs& g, const void* p, int c, int ld) { g.a0 = p; g.c0 = c; g.lda0 = ld; }
inline void ga_rows(GemmArgs& g, const Act& x) { ga_rows(g, x.p, x.C, x.C); }
inline void ga_rows2(GemmArgs& g, const void* p, int c, int ld) { g.a1 = p; g.c1 = c; g.lda1 = ld; }  // second concat source
inline void ga_rows2(GemmArgs& g, const Act* x1) { if (x1) ga_rows2(g, x1->p, x1->C, x1->C); }
// 3x3 conv over [B][H][W] images: Hout / Wout follow from stride and the x2 up-sampling (nearest, or zero-stuffed: a stride-2 conv's dgrad)
inline void ga_conv3(GemmArgs& g, int B, int H, int W, int stride = 1, int ups = 0, int pad = 1, int zstuff = 0) {
    g.conv = 1; g.B = B; g.Hin = H; g.Win = W; g.Hout = ((H << ups) - 1) / stride + 1; g.Wout = ((W << ups) - 1) / stride + 1;
    g.stride = stride; g.ups = ups; g.pad = pad; g.zstuff = zstuff;
}
inline void ga_conv3(GemmArgs& g, const Act& x, int stride = 1, int ups = 0, int pad = 1, int zstuff = 0) { ga_conv3(g, x.B, x.H, x.W, stride, ups, pad, zstuff); }
// the 1x1 tail of a 3x3 conv: row sources read at the output pixel
inline void ga_tail(GemmArgs& g, const void* p, int c, int ld) { g.s0 = p; g.cs0 = c; g.lds0 = ld; }
inline void ga_tail2(GemmArgs& g, const void* p, int c, int ld) { g.s1 = p; g.cs1 = c; g.lds1 = ld; }
// ---- W operand and the problem size ----
inline void ga_weight(GemmArgs& g, const void* w, int M, int N, int K) { g.w = w; g.M = M; g.N = N; g.K = K; }
// ---- batching: element strides per batch index; with heads, output offset = (z / heads) * o_bs + (z % heads) * o_hs ----
inline void ga_batch(GemmArgs& g, int batch, long long a_bs, long long w_bs, long long o_bs) { g.batch = batch; g.a_bs = a_bs; g.w_bs = w_bs; g.o_bs = o_bs; }
inline void ga_batch_heads(GemmArgs& g, int batch, long long a_bs, long long w_bs, int heads, long long o_bs, long long o_hs) {
    ga_batch(g, batch, a_bs, w_bs, o_bs);
    g.heads = heads; g.o_hs = o_hs;
}
// ---- output and epilogue ----
inline void ga_out(GemmArgs& g, void* out, int ldo) { g.out = out; g.ldo = ldo; }
inline void ga_out_f32(GemmArgs& g, float* out, int ldo) { g.out_mode = OUT_F32; g.out = out; g.ldo = ldo; }
inline void ga_resid(GemmArgs& g, const void* p, int ldr) { g.resid = p; g.ldr = ldr; }
inline void ga_resid(GemmArgs& g, const Act* r) { if (r) ga_resid(g, r->p, r->C); }
inline void ga_rowvec(GemmArgs& g, const float* rowvec, int ld, int div) { g.rowvec = rowvec; g.rowvec_ld = ld; g.rowvec_div = div; }
// out[m][n] += sum_q z[m][(n / secN) * r + q] * b[n][q], z f32 of pitch zld from an earlier pass
inline void ga_lora_epilogue(GemmArgs& g, const float* z, int zld, const float* b, int r, int secN) {
    g.lora_z = z; g.lora_zld = zld; g.lora_b = b; g.lora_r = r; g.lora_secN = secN;
}
inline void ga_lora_epilogue(GemmArgs& g, const ConvW& cw, const float* z) { ga_lora_epilogue(g, z, cw.r, cw.loraB, cw.r, cw.cout); }

// ---- plan, allocate, launch ----
// an allocator is any callable void*(size_t) whose memory outlives the stream work; null = failure
inline size_t gemm_partial_bytes(const GemmArgs& g) { return (size_t)g.splitk * g.batch * g.M * g.N * sizeof(float); }
template <typename Alloc>
int gemm_alloc_partial(GemmArgs& g, Alloc&& alloc) {  // the f32 slabs of a planned launch (a site that launches later calls this itself)
    if (g.splitk <= 1) return 0;
    g.partial = static_cast<float*>(alloc(gemm_partial_bytes(g)));
    return g.partial ? 0 : 7;
}
template <typename T, typename Alloc>
int gemm_finish(GemmArgs& g, hipStream_t st, bool dry, Alloc&& alloc) {  // of a launch whose plan the caller made (and may have acted on)
    TRY(gemm_alloc_partial(g, alloc));
    if (dry) return 0;
    return launch_gemm<T>(g, st);
}
template <typename T, typename Alloc>
int gemm_run(GemmArgs& g, hipStream_t st, bool dry, Alloc&& alloc) {
    TRY(gemm_choose(g, sizeof(T) == 2));
    return gemm_finish<T>(g, st, dry, alloc);
}
inline auto devbuf_alloc(DevBuf& b) {  // one DevBuf as the allocator of one launch (grows, never shrinks)
    return [&b](size_t n) -> void* { return b.reserve(n, false) ? nullptr : b.p; };
}

// ---- a resnet's GEMMs ----
// conv2(hn) + bias + resid -> out.  tail_cin > 0: the 1x1 shortcut on the raw input [x | x1] (tail_cin channels) rides as the tail of the
// K loop instead, on the bank [W_c2 | W_sc] with the summed bias (`w` / `bias` are that bank's), and there is no residual
inline GemmArgs resnet_conv2_args(const void* hn, int B, int H, int W, int cout, const void* w, const float* bias, const void* resid, void* out,
                                  int tail_cin = 0, const Act* x = nullptr, const Act* x1 = nullptr) {
    GemmArgs g;
    ga_rows(g, hn, cout, cout);
    ga_conv3(g, B, H, W);
    if (tail_cin) {
        ga_tail(g, x->p, x->C, x->C);
        if (x1) ga_tail2(g, x1->p, x1->C, x1->C);
    } else {
        ga_resid(g, resid, cout);
    }
    ga_weight(g, w, B * H * W, cout, 9 * cout + tail_cin);
    g.bias = bias;
    ga_out(g, out, cout);
    return g;
}
// the 1x1 shortcut on the (concatenated) raw input, written to `out`
inline GemmArgs resnet_shortcut_args(const Act& x, const Act* x1, const void* w, const float* bias, int cin, int cout, void* out) {
    GemmArgs g;
    ga_rows(g, x);
    ga_rows2(g, x1);
    ga_weight(g, w, (int)x.rows(), cout, cin);
    g.bias = bias;
    ga_out(g, out, cout);
    return g;
}

// ---- attention core on head-major operands: q [B*H][npad][dpad], k [B*H][nkpad][dpad], vt [B*H][dpad][nkpad] -> out rows [B][N][H*hd] ----
struct AttnGeom { int B = 0, H = 0, N = 0, npad = 0, hd = 0, dpad = 0, nk = 0, nkpad = 0; };
inline float attn_scale(int hd) { return 1.0f / sqrtf((float)hd); }
// the flash path's arguments; fp8: the e4m3 K / V^T and the per-head scales come from `alloc` (in that order)
template <typename Alloc>
int attn_flash_args(AttnArgs& a, const AttnGeom& s, const void* q, const void* k, const void* vt, void* out, float* lse, bool fp8, Alloc&& alloc) {
    a.q = q; a.k = k; a.vt = vt; a.out = out;
    a.B = s.B; a.H = s.H; a.nq = s.N; a.nk = s.nk; a.nkpad = s.nkpad; a.hd = s.hd; a.dpad = s.dpad;
    a.scale = attn_scale(s.hd); a.lse = lse;
    if (!fp8) return 0;
    const size_t b8 = (size_t)s.B * s.H * s.nkpad * s.dpad;
    a.k8 = alloc(b8);
    a.vt8 = alloc(b8);
    a.f8_scales = static_cast<float*>(alloc((size_t)s.B * s.H * 4 * sizeof(float)));
    return a.k8 && a.vt8 && a.f8_scales ? 0 : 7;
}
inline int attn_flash_launch(const AttnArgs& a, bool fp8, bool dry, hipStream_t st) {
    if (dry) return 0;
    return fp8 ? launch_attention_fp8(a, st) : launch_attention_bf16(a, st);
}
// the materialised sequence: S = scale Q K^T (f32), P = softmax(S) as T (f32: P == S, in place), out = P V.  S and P are the caller's,
// [B*H][N][nkpad] each - who allocates them decides what outlives the call; run(GemmArgs&) plans and (unless dry) launches one GEMM
template <typename T, typename RunGemm>
int attn_materialised(const AttnGeom& s, const void* q, const void* k, const void* vt, float* S, void* P, void* out_rows, bool dry, hipStream_t st,
                      RunGemm&& run) {
    const int BH = s.B * s.H;
    const long long sn = (long long)s.N * s.nkpad;
    GemmArgs g;
    ga_rows(g, q, s.dpad, s.dpad);
    ga_weight(g, k, s.N, s.nkpad, s.dpad);
    ga_batch(g, BH, (long long)s.npad * s.dpad, (long long)s.nkpad * s.dpad, sn);
    g.alpha = attn_scale(s.hd);
    ga_out_f32(g, S, s.nkpad);
    TRY(run(g));
    if (!dry) TRY(launch_softmax_rows<T>(S, s.nkpad, P, s.nkpad, (long long)BH * s.N, s.nk, st));
    GemmArgs o;
    ga_rows(o, P, s.nkpad, s.nkpad);
    ga_weight(o, vt, s.N, s.hd, s.nkpad);
    ga_batch_heads(o, BH, sn, (long long)s.dpad * s.nkpad, s.H, (long long)s.N * s.H * s.hd, s.hd);
    ga_out(o, out_rows, s.H * s.hd);
    return run(o);
}

}  // namespace mrisr
