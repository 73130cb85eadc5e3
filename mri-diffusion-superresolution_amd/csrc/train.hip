// LoRA fine-tuning step of the denoiser (reference: the training cell of the ResDif notebook,
// nb:ResDif c11:14-41 - loss = mse(eps_hat, eps), backward for the adapters only, clip 1.0, AdamW).
//
// Forward: the same launch sequence as inference (runner.h), run with Model::keep so nothing is recycled, with P of
// every attention materialised and every block recording what its backward needs.  Backward: the recorded blocks are
// replayed in reverse.  Base weights are frozen, so the backward is dX everywhere (dgrad GEMMs on transposed / tap-flipped
// weight copies packed once by train_prepare) plus the rank-r wgrads of the adapters, accumulated with float atomics
// into the caller's flat f32 gradient vector (which the host all-reduces over RCCL before the optimiser step).
#include <algorithm>
#include <functional>
#include <set>

#include "model.h"
#include "runner.h"
#include "train_ops.h"

namespace mrisr {

// ================================================================================================
// load-time packing for the backward
// ================================================================================================
// adapter of fused-module slot `slot` (theta: A [r][k], B [n][r]) -> the four device views the kernels read:
//   loraA [R][k] T (forward down-projection), loraAT [k][R] f32 (dgrad epilogue),
//   loraB [ntot][r] f32 = s*B (forward epilogue), loraBT [R][ntot] T = s*B^T (backward down-projection)
// half > 0 (ff.net.0.proj, n = 2 * half): theta keeps B in raw row order (value half, then gate half); the views are written in
// the packed weight's row order, (value, gate) interleaved in blocks of 16
template <typename T>
__global__ void lora_refresh_kernel(const float* __restrict__ A, const float* __restrict__ B, T* loraA, float* loraAT, float* loraB,
                                    T* loraBT, int r, int R, int k, int n, int ntot, int slot, int row0, float s, int half) {
    const long long na = (long long)r * k, nb = (long long)n * r;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256) {
        if (i < na) {
            const int q = (int)(i / k), c = (int)(i - (long long)q * k);
            const float v = A[i];
            loraA[(size_t)(slot * r + q) * k + c] = from_f32<T>(v);
            loraAT[(size_t)c * R + slot * r + q] = v;
        } else {
            const long long j = i - na;
            const int c = (int)(j / r), q = (int)(j - (long long)c * r);
            const float v = s * B[j];
            const int row = row0 + (half ? geglu_packed_row(c, half) : c);
            loraB[(size_t)row * r + q] = v;
            loraBT[(size_t)(slot * r + q) * ntot + row] = from_f32<T>(v);
        }
    }
}

// rank 32 .. 128: the same adapter into the packed layout - loraA [R][k], the sB columns of w [n][k + R], loraBT [R][ntot]
// and the A^T columns of wT [k][ntot + R]; module `slot`'s rank-r block sits at slot * rp (the padding up to rp stays zero)
template <typename T>
__global__ void lora_refresh_hr_kernel(const float* __restrict__ A, const float* __restrict__ B, T* loraA, T* w, T* loraBT, T* wT, int r, int rp,
                                       int R, int k, int n, int ntot, int slot, int row0, float s, int half) {
    const long long na = (long long)r * k, nb = (long long)n * r;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < na + nb; i += (long long)gridDim.x * 256) {
        if (i < na) {
            const int q = (int)(i / k), c = (int)(i - (long long)q * k);
            const T v = from_f32<T>(A[i]);
            loraA[(size_t)(slot * rp + q) * k + c] = v;
            if (wT) wT[(size_t)c * (ntot + R) + ntot + slot * rp + q] = v;  // (no dgrad bank: the context projections)
        } else {
            const long long j = i - na;
            const int c = (int)(j / r), q = (int)(j - (long long)c * r);
            const T v = from_f32<T>(s * B[j]);
            const int row = row0 + (half ? geglu_packed_row(c, half) : c);
            w[(size_t)row * (k + R) + k + slot * rp + q] = v;
            loraBT[(size_t)(slot * rp + q) * ntot + row] = v;
        }
    }
}

template <typename F>
static void for_each_xf(Model& m, F f) {
    for (auto& lv : m.down) for (auto& x : lv.xf) f(x);
    f(m.mid_xf);
    for (auto& lv : m.up) for (auto& x : lv.xf) f(x);
}
template <typename F>
static void for_each_res(Model& m, F f) {
    for (auto& lv : m.down) for (auto& r : lv.res) f(r);
    f(m.mid_r0);
    f(m.mid_r1);
    for (auto& lv : m.up) for (auto& r : lv.res) f(r);
}

std::vector<LinW*> Model::lora_linears() {
    std::vector<LinW*> v;
    for_each_xf(*this, [&](XfW& x) {
        for (LinW* l : {&x.proj_in, &x.qkv, &x.out1, &x.q2, &x.kv2, &x.out2, &x.ff1, &x.ff2, &x.proj_out})
            if (l->R) v.push_back(l);
    });
    return v;
}

std::vector<ConvW*> Model::lora_convs() {
    std::vector<ConvW*> v;
    for_each_res(*this, [&](ResW& r) {
        if (r.c1.r) v.push_back(&r.c1);
        if (r.c2.r) v.push_back(&r.c2);
    });
    return v;
}

// the backward's copies of one layer's weights (both prepare functions below); err keeps the last failure
// wd[ci][ky][kx][co] = w[co][ci][2-ky][2-kx]: the dgrad of a 3x3 conv is a 3x3 conv of dY with this bank
template <typename T>
static void pack_conv_dgrad(Model& m, ConvW& c, hipStream_t st, int& err) {
    if (!c.w || c.ks != 3 || c.wd) return;
    const RawParam* w = m.find(c.name + ".weight");
    if (!w) { err = 3; set_error("missing parameter: " + c.name + ".weight"); return; }
    c.wd = m.new_packed((size_t)w->numel() * sizeof(T), false);
    if (!c.wd) { err = 4; return; }
    if (launch_pack_conv_dgrad<T>(static_cast<const float*>(w->data->p), c.wd, c.cout, c.cin, st)) err = 5;
}
// wT = w^T.  repack: a linear that already has its wT is transposed again into the same buffer (full-parameter training: the weights
// change every step); otherwise it is left alone (frozen base weights)
template <typename T>
static void pack_lin_t(Model& m, LinW& l, bool repack, hipStream_t st, int& err) {
    if (!l.w || (l.wT && !repack)) return;
    const int ldt = l.rp ? l.n + l.R : l.n;  // high rank: [k][n + R] = [W^T | A^T], the A^T columns written by lora_refresh
    if (!l.wT) l.wT = m.new_packed((size_t)ldt * l.k * sizeof(T), l.rp != 0);
    if (!l.wT) { err = 4; return; }
    if (launch_transpose<T>(l.w, l.wT, l.n, l.k, l.kw(), ldt, 0, 0, 1, l.n, st)) err = 5;
}

template <typename T>
static int train_prepare_t(Model& m, hipStream_t st) {
    int err = 0;
    auto conv_dgrad = [&](ConvW& c) { pack_conv_dgrad<T>(m, c, st, err); };
    auto lin_t = [&](LinW& l) { pack_lin_t<T>(m, l, false, st, err); };
    for_each_res(m, [&](ResW& r) {
        conv_dgrad(r.c1);
        conv_dgrad(r.c2);
        if (r.has_sc) lin_t(r.sc);
    });
    for (auto& lv : m.down) if (lv.has_down) conv_dgrad(lv.down);
    for (auto& lv : m.up) if (lv.has_up) conv_dgrad(lv.up);
    conv_dgrad(m.conv_out);
    for_each_xf(m, [&](XfW& x) {
        for (LinW* l : {&x.proj_in, &x.qkv, &x.out1, &x.q2, &x.out2, &x.ff1, &x.ff2, &x.proj_out}) lin_t(*l);
        // the fp8 forward of the step has no adapted GEGLU projection: refuse before any step runs in another precision
        if (x.ff1.R && m.cfg.fp8_train) { err = 6; set_error("fp8_train does not cover LoRA on ff.net.0.proj: train this handle without fp8_train"); }
        if (x.ff1.R && x.ff1.geglu_half % 16 != 0) { err = 6; set_error("LoRA on ff.net.0.proj: the (value, gate) interleave is 16 rows wide"); }
    });
    if (err) return err;
    // flat trainable vector: [A_0 | B_0 | A_1 | B_1 ...] in lora_linears() x fused-module order
    m.trainables.clear();
    long long off = 0;
    for (LinW* l : m.lora_linears()) {
        const int nmod = (int)l->mod_names.size();
        l->offA.assign(nmod, -1);
        l->offB.assign(nmod, -1);
        for (int j = 0; j < nmod; ++j) {
            if (!l->mod_lora[j]) continue;
            l->offA[j] = off;
            m.trainables.push_back({l->mod_names[j] + ".lora_A.default.weight", off, (long long)l->r * l->k, l->r, l->k});
            off += (long long)l->r * l->k;
            l->offB[j] = off;
            m.trainables.push_back({l->mod_names[j] + ".lora_B.default.weight", off, (long long)l->secN * l->r, l->secN, l->r});
            off += (long long)l->secN * l->r;
        }
        if (!l->loraBT) {
            l->loraBT = m.new_packed((size_t)l->R * l->n * sizeof(T), true);
            if (!l->rp) l->loraAT = static_cast<float*>(m.new_packed((size_t)l->k * l->R * sizeof(float), true));
            if (!l->loraBT || (!l->rp && !l->loraAT)) return 4;
        }
    }
    // conv adapters follow ALL linear adapters (whose offsets are therefore the same with and without them): resnets in walk order,
    // conv1 A, B, then conv2 A, B; tensors in PyTorch's 4-D shapes
    for (ConvW* c : m.lora_convs()) {
        Model::Trainable ta{c->name + ".lora_A.default.weight", off, (long long)c->r * c->cin * 9, c->r, c->cin * 9};
        ta.ndim = 4; ta.shape[0] = c->r; ta.shape[1] = c->cin; ta.shape[2] = 3; ta.shape[3] = 3;
        c->offLA = off;
        m.trainables.push_back(ta);
        off += ta.numel;
        Model::Trainable tb{c->name + ".lora_B.default.weight", off, (long long)c->cout * c->r, c->cout, c->r};
        tb.ndim = 4; tb.shape[0] = c->cout; tb.shape[1] = c->r; tb.shape[2] = 1; tb.shape[3] = 1;
        c->offLB = off;
        m.trainables.push_back(tb);
        off += tb.numel;
    }
    // DoRA magnitudes follow ALL lora_A / lora_B tensors (whose offsets therefore do not depend on the flag): 1-D [out_features] per adapted
    // module, in PyTorch's row order
    for (LinW* l : m.lora_linears()) {
        l->offM.assign(l->mod_names.size(), -1);
        if (!l->dora_g) continue;
        for (size_t j = 0; j < l->mod_names.size(); ++j) {
            if (!l->mod_lora[j]) continue;
            Model::Trainable tm{l->mod_names[j] + ".lora_magnitude_vector.default.weight", off, (long long)l->secN, l->secN, 1};
            tm.ndim = 1; tm.shape[0] = l->secN; tm.shape[1] = tm.shape[2] = tm.shape[3] = 1;
            l->offM[j] = off;
            m.trainables.push_back(tm);
            off += l->secN;
        }
    }
    m.n_trainable = off;
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    m.train_ready = true;
    return 0;
}

int Model::train_prepare(hipStream_t st) {
    MRISR_REQUIRE(finalized, "call mrisr_model_finalize first");
    MRISR_REQUIRE(!is_controlnet, "the fine-tuning step is implemented for the UNet handle");
    // lora_rank == 0: a FROZEN UNet - the step then only differentiates with respect to its inputs (ControlNet residuals,
    // T2I-Adapter features): no trainable vector, dX only
    MRISR_REQUIRE(cfg.lora_rank == 0 || cfg.lora_fused, "fine-tuning needs explicit (un-merged) LoRA adapters");
    if (train_ready) return 0;
    return cfg.compute_dtype == MRISR_F32 ? train_prepare_t<float>(*this, st) : train_prepare_t<bf16>(*this, st);
}

int Model::train_bind(float* theta_dev, float* grad_dev, hipStream_t st) {
    TRY(train_prepare(st));
    MRISR_REQUIRE(n_trainable == 0 || (theta_dev && grad_dev), "theta / grad device buffers");
    theta = theta_dev;
    grad = grad_dev;
    return 0;
}

// DoRA, after the adapter views of `l` are written from theta: g = m / ||W + s B A|| from the f32 masters, then everything the
// forward and the backward multiply by carries it - the rows of w (g W), the B views (g s B: loraB / the sB columns, loraBT) and the W^T part
// of wT.  The A views stay as they are.  Launches only.
template <typename T>
static int dora_refresh_t(Model& m, LinW& l, hipStream_t st) {
    int row0 = 0;
    for (size_t j = 0; j < l.mod_names.size(); ++j, row0 += l.secN) {
        if (!l.mod_lora[j]) continue;
        const RawParam* w = m.find(l.mod_names[j] + ".weight");
        MRISR_REQUIRE(w && l.offM[j] >= 0 && w->numel() == (int64_t)l.secN * l.k, "DoRA refresh: master weight / magnitude of " + l.mod_names[j]);
        const float* A = m.theta + l.offA[j];
        const float* B = m.theta + l.offB[j];
        TRY(launch_dora_scale<T>(static_cast<const float*>(w->data->p), A, B, m.theta + l.offM[j], m.lora_scale, l.dora_g, l.w, l.kw(), row0, l.secN,
                                 l.k, l.r, l.geglu_half, 0, st));
        TRY(launch_dora_refresh_b<T>(B, l.dora_g, m.lora_scale, l.rp ? nullptr : l.loraB_rw, l.rp ? l.w : nullptr, l.kw(),
                                     l.rp ? lora_hr_wcol(l.k, (int)j, l.rp) : 0, l.loraBT, l.n, (int)j * (l.rp ? l.rp : l.r), row0, l.secN, l.r,
                                     l.geglu_half, st));
    }
    if (l.wT) TRY(launch_transpose<T>(l.w, l.wT, l.n, l.k, l.kw(), l.rp ? l.n + l.R : l.n, 0, 0, 1, l.n, st));
    return 0;
}

int Model::lora_refresh(hipStream_t st) {
    MRISR_REQUIRE(train_ready && (theta || n_trainable == 0), "bind the trainable vector first");
    for (LinW* l : lora_linears()) {
        int row0 = 0;
        for (size_t j = 0; j < l->mod_names.size(); ++j, row0 += l->secN) {
            if (!l->mod_lora[j]) continue;
            const float* A = theta + l->offA[j];
            const float* B = theta + l->offB[j];
            const long long total = (long long)l->r * l->k + (long long)l->secN * l->r;
            const unsigned blocks = (unsigned)((total + 255) / 256);
            if (l->rp) {  // the same launch refreshes the sB columns of w and the A^T columns of wT
                if (cfg.compute_dtype == MRISR_F32)
                    hipLaunchKernelGGL(lora_refresh_hr_kernel<float>, dim3(blocks), dim3(256), 0, st, A, B, static_cast<float*>(l->loraA), static_cast<float*>(l->w),
                                       static_cast<float*>(l->loraBT), static_cast<float*>(l->wT), l->r, l->rp, l->R, l->k, l->secN, l->n, (int)j, row0, lora_scale, l->geglu_half);
                else
                    hipLaunchKernelGGL(lora_refresh_hr_kernel<bf16>, dim3(blocks), dim3(256), 0, st, A, B, static_cast<bf16*>(l->loraA), static_cast<bf16*>(l->w),
                                       static_cast<bf16*>(l->loraBT), static_cast<bf16*>(l->wT), l->r, l->rp, l->R, l->k, l->secN, l->n, (int)j, row0, lora_scale, l->geglu_half);
                continue;
            }
            if (cfg.compute_dtype == MRISR_F32)
                hipLaunchKernelGGL(lora_refresh_kernel<float>, dim3(blocks), dim3(256), 0, st, A, B, static_cast<float*>(l->loraA), l->loraAT,
                                   l->loraB_rw, static_cast<float*>(l->loraBT), l->r, l->R, l->k, l->secN, l->n, (int)j, row0, lora_scale, l->geglu_half);
            else
                hipLaunchKernelGGL(lora_refresh_kernel<bf16>, dim3(blocks), dim3(256), 0, st, A, B, static_cast<bf16*>(l->loraA), l->loraAT,
                                   l->loraB_rw, static_cast<bf16*>(l->loraBT), l->r, l->R, l->k, l->secN, l->n, (int)j, row0, lora_scale, l->geglu_half);
        }
        if (l->dora_g) TRY(cfg.compute_dtype == MRISR_F32 ? dora_refresh_t<float>(*this, *l, st) : dora_refresh_t<bf16>(*this, *l, st));
        // the fp8 copy of the adapters' A rows (inference through the fp8 projections after training steps)
        if (l->loraA8 && cfg.compute_dtype != MRISR_F32) TRY(launch_quant_rows_fp8(l->loraA, l->R, l->k, l->loraA8, l->loraA_scale, st));
    }
    for (ConvW* c : lora_convs()) {
        const float* A = theta + c->offLA;
        const float* B = theta + c->offLB;
        if (cfg.compute_dtype == MRISR_F32) TRY(launch_conv_lora_pack<float>(A, B, lora_scale, c->loraA, c->loraAd, c->loraB, c->loraBT, c->cin, c->cout, c->r, st));
        else TRY(launch_conv_lora_pack<bf16>(A, B, lora_scale, c->loraA, c->loraAd, c->loraB, c->loraBT, c->cin, c->cout, c->r, st));
    }
    // the K-permuted copies the fused middle reads (bf16, C = 320) follow the rows of a DoRA projection
    if (dora) {
        int rc = 0;
        for_each_xf(*this, [&](XfW& x) {
            if (x.q2p && x.q2.dora_g && !rc) rc = launch_pack_mlp_w2(x.q2.w, x.q2p, x.q2.n, x.q2.k, st);
            if (x.out2p && x.out2.dora_g && !rc) rc = launch_pack_mlp_w2(x.out2.w, x.out2p, x.out2.n, x.out2.k, st);
        });
        TRY(rc);
    }
    MRISR_CHECK_HIP(hipGetLastError());
    ctx_valid = false;  // cached cross-attention K / V depend on attn2.to_k / to_v adapters
    return 0;
}

// ================================================================================================
// the step
// ================================================================================================
template <typename T>
struct Trainer : Runner<T> {
    typedef Runner<T> R;
    using R::m;
    using R::st;
    using R::dry;
    using R::alloc;
    using R::new_act;
    static constexpr int BK = 128 / (int)sizeof(T);

    struct Slot { void* g = nullptr; bool written = false; };
    std::map<const void*, Slot> slots;   // activation -> its gradient buffer
    std::set<const void*> live;          // activations downstream of a trainable parameter
    std::vector<std::function<int()>> tape;
    std::map<const XfW*, float*> z_kv;   // adapter down-projections of the cached context K / V
    std::map<const XfW*, const void*> y_kv;  // DoRA: the context K / V projections as rows [B * L][2C] (the cache itself is head-major)

    Trainer(Model& mm, hipStream_t s, bool d) : R(mm, s, d) {}

    Slot& slot(const Act& a) {
        auto it = slots.find(a.p);
        if (it == slots.end()) {
            Slot s;
            s.g = alloc(a.numel() * sizeof(T));
            it = slots.insert({a.p, s}).first;
        }
        return it->second;
    }
    bool is_live(const Act& a) const { return live.count(a.p) != 0; }
    int zero(void* p, size_t bytes) {
        if (!p) return 7;
        if (dry) return 0;
        MRISR_CHECK_HIP(hipMemsetAsync(p, 0, bytes, st));
        return 0;
    }
    static bool has_lora(const XfW& x) {
        return x.proj_in.R || x.qkv.R || x.out1.R || x.q2.R || x.kv2.R || x.out2.R || x.ff1.R || x.ff2.R || x.proj_out.R;
    }

    // ---------------------------------------------------------------------------------------------
    // backward building blocks
    // ---------------------------------------------------------------------------------------------
    // ---------------------------------------------------------------------------------------------
    // full-parameter training (m.full_grad bound: ControlNet): weight / bias gradients of every conv and linear, accumulated into
    // the caller's flat f32 vector at the raw tensor's offset (PyTorch layouts).  One pixel-contraction GEMM per layer,
    //     dW[co][tap * cin + ci] = sum_m dY^T[co][m] . im2col^T[tap * cin + ci][m]
    // (a linear / 1 x 1 conv is the ks = 1 case), then one scatter-add; db by column sums.
    // ---------------------------------------------------------------------------------------------
    bool full() const { return m.full_grad != nullptr; }
    float* gptr(const std::string& key) const {
        auto it = m.full_off.find(key);
        return it == m.full_off.end() ? nullptr : m.full_grad + it->second;
    }
    // x: NHWC [xB][xH][xW][cin_src] (rows [M][cin_src] for a linear: xB = 1, xH = M, xW = 1); dY: rows [M][.] of pitch ldy, columns
    // col0 .. col0 + cout_src; the raw tensor is [cout][cin][ks][ks] with cout <= cout_src, cin <= cin_src (zero-padded layers).
    int wgrad(const void* x, int xB, int xH, int xW, int cin_src, const void* dY, int ldy, int col0, int Ho, int Wo, int cout_src, int ks,
              int stride, float* gW, float* gB, int cout, int cin, int geglu_half = 0) {
        const size_t mk = m.arena.mark();
        TRY(conv_wgrad_run<T>(st, dry, [this](size_t n) { return alloc(n); }, [this](GemmArgs& g) { return R::run_gemm(g); }, x, xB, xH, xW,
                              cin_src, dY, ldy, col0, Ho, Wo, cout_src, ks, stride, gW, gB, cout, cin, geglu_half));
        m.arena.release(mk);
        return 0;
    }
    int wgrad_conv(const Act& x, const Act& dy, const ConvW& cw, int stride) {
        if (!full()) return 0;
        const RawParam* w = m.find(cw.name + ".weight");
        MRISR_REQUIRE(w && dy.C == cw.cout && x.C == cw.cin, "conv weight gradient: operands");
        return wgrad(x.p, x.B, x.H, x.W, x.C, dy.p, dy.C, 0, dy.H, dy.W, dy.C, cw.ks, stride, gptr(cw.name + ".weight"), gptr(cw.name + ".bias"),
                     (int)w->shape[0], (int)w->shape[1]);
    }
    // a (possibly fused) linear: one gradient GEMM per fused module on its column section of dY
    int wgrad_linear(const LinW& lw, const void* x, int ldx, const void* dY, int ldy, int M) {
        if (!full()) return 0;
        MRISR_REQUIRE(ldx == lw.k && !lw.mod_names.empty(), "linear weight gradient: contiguous input rows of a named module");
        const int nmod = (int)lw.mod_names.size(), secN = lw.n / nmod;
        for (int j = 0; j < nmod; ++j) {
            const std::string& name = lw.mod_names[j];
            const bool geglu = name.size() > 13 && name.compare(name.size() - 13, 13, "ff.net.0.proj") == 0;
            TRY(wgrad(x, 1, M, 1, lw.k, dY, ldy, j * secN, M, 1, secN, 1, 1, gptr(name + ".weight"), gptr(name + ".bias"), secN, lw.k,
                      geglu ? secN / 2 : 0));
        }
        return 0;
    }

    // affine parameters of a GroupNorm(+SiLU) / LayerNorm (dy: gradient with respect to the norm's OUTPUT)
    int gn_affine(const Act& x, const void* dy, const NormW& nw, bool silu, float eps, const float* fwd_partial, int nsplit) {
        if (!full() || dry) return 0;
        float* gg = gptr(nw.name + ".weight");
        float* gb = gptr(nw.name + ".bias");
        MRISR_REQUIRE(gg && gb && nw.c == x.C, "GroupNorm affine gradient: parameters");
        return launch_gn_affine_grad<T>(x.p, dy, nw.g, nw.b, fwd_partial, nsplit, m.cfg.norm_num_groups, x.B, x.H * x.W, x.C, eps, silu ? 1 : 0, gg, gb, st);
    }
    int ln_affine(const void* x, const void* dy, const NormW& nw, int M, int C) {
        if (!full() || dry) return 0;
        float* gg = gptr(nw.name + ".weight");
        float* gb = gptr(nw.name + ".bias");
        MRISR_REQUIRE(gg && gb, "LayerNorm affine gradient: parameters");
        return launch_ln_affine_grad<T>(x, dy, M, C, 1e-5f, gg, gb, st);
    }
    // the time-embedding path, after every ResnetBlock has added its share to m.d_tproj:  tproj_out = Wp silu(emb) + bp,
    // emb = W2 silu(y1) + b2,  y1 = W1 s + b1  (Runner::time_embed); rows = 1 (scalar timestep) or B
    int time_embed_bwd(int B) {
        if (!full()) return 0;
        const int rows = m.t_scalar ? 1 : B, c0 = m.cfg.block_out_channels[0], temb = 4 * c0;
        const size_t mk = m.arena.mark();
        float* d_emb = static_cast<float*>(alloc((size_t)rows * temb * sizeof(float)));
        float* d_y1 = static_cast<float*>(alloc((size_t)rows * temb * sizeof(float)));
        if (!d_emb || !d_y1) return 7;
        if (!dry) {
            int off = 0;
            for (auto& mod : m.temb_mods) {
                const RawParam* w = m.find(mod + ".weight");
                MRISR_REQUIRE(w, "time_emb_proj weight");
                const int n = (int)w->shape[0];
                TRY(launch_small_wgrad(m.d_tproj + off, m.tproj_total, m.te_emb, temb, rows, n, temb, 1, gptr(mod + ".weight"), gptr(mod + ".bias"), st));
                off += n;
            }
            TRY(launch_small_dgrad<T>(m.d_tproj, m.tproj_total, m.tproj.w, rows, m.tproj_total, temb, m.te_emb, temb, d_emb, temb, st));
            TRY(launch_small_wgrad(d_emb, temb, m.te_y1, temb, rows, temb, temb, 1, gptr("time_embedding.linear_2.weight"), gptr("time_embedding.linear_2.bias"), st));
            TRY(launch_small_dgrad<T>(d_emb, temb, m.te2.w, rows, temb, temb, m.te_y1, temb, d_y1, temb, st));
            TRY(launch_small_wgrad(d_y1, temb, m.te_s, c0, rows, temb, c0, 0, gptr("time_embedding.linear_1.weight"), gptr("time_embedding.linear_1.bias"), st));
        }
        m.arena.release(mk);
        return 0;
    }

    // dX (+)= conv3x3(dY, wd).  mode 1: the forward conv had stride 2 -> dY is zero-stuffed to twice its size
    int conv_dgrad(const Act& dy, const ConvW& cw, int mode, void* out, bool acc) {
        MRISR_REQUIRE(cw.wd && dy.C == cw.cout, "conv dgrad weights");
        return conv_dgrad_run<T>(st, dry, [this](GemmArgs& g) { return R::run_gemm(g); }, dy.p, dy.B, dy.H, dy.W, cw.cout, cw.cin, cw.wd,
                                 mode, out, acc ? out : nullptr, cw.cin);
    }

    int gn_bwd(const Act& x0, const Act* x1, const NormW& nw, bool silu, float eps, const float* fwd_partial, int nsplit,
               const void* dy, void* dx0, bool acc0, void* dx1, bool acc1) {
        GroupNormBwdArgs a;
        a.x0 = x0.p; a.c0 = x0.C;
        a.x1 = x1 ? x1->p : nullptr; a.c1 = x1 ? x1->C : 0;
        a.B = x0.B; a.HW = x0.H * x0.W; a.groups = m.cfg.norm_num_groups; a.eps = eps;
        a.gamma = nw.g; a.beta = nw.b; a.silu = silu ? 1 : 0;
        a.dy = dy; a.dx0 = dx0; a.dx1 = dx1; a.acc0 = acc0 ? 1 : 0; a.acc1 = acc1 ? 1 : 0;
        a.fwd_partial = fwd_partial; a.nsplit = nsplit;
        a.bwd_partial = static_cast<float*>(alloc((size_t)a.B * nsplit * a.groups * 2 * sizeof(float)));
        if (!a.bwd_partial) return 7;
        if (dry) return 0;
        return launch_groupnorm_bwd<T>(a, st);
    }

    // backward of y = x W^T + s B (A x):  dX (+)= dY W + (dY s B) A;  dA, dB accumulated into m.grad
    // DoRA (lw.dora_g): the operands are already the scaled ones, so dz, dA and dX come out right as they are; this call's dB is reduced
    // into scratch and enters the gradient with row j scaled by g[j] (dora_b_begin / dora_b_end), and the magnitude's gradient needs the
    // projection's own output: yout (rows [M][n] of pitch ldyo, as the epilogue wrote them) and the residual yres it added (null: none)
    int dora_b_begin(const LinW& lw, float** tmp) {  // zeroed scratch: module j's [secN][r] block at j * secN * r
        const size_t bytes = lw.mod_names.size() * (size_t)lw.secN * lw.r * sizeof(float);
        *tmp = static_cast<float*>(alloc(bytes));
        if (!*tmp) return 7;
        return zero(*tmp, bytes);
    }
    int dora_b_end(const LinW& lw, const float* tmp) {
        const int nmod = (int)lw.mod_names.size();
        const size_t per = (size_t)lw.secN * lw.r;
        for (int j = 0; j < nmod; ++j)
            if (lw.mod_lora[j]) TRY(launch_dora_rowscale_add(tmp + j * per, lw.dora_g, m.grad + lw.offB[j], j * lw.secN, lw.secN, lw.r, lw.geglu_half, st));
        return 0;
    }
    int dora_mag_bwd(const LinW& lw, const void* dY, int ldy, int M, const void* yout, int ldyo, const void* yres, int ldres) {
        MRISR_REQUIRE(yout && m.grad && m.theta, "DoRA backward: the projection's output rows");
        const int nmod = (int)lw.mod_names.size();
        float* scratch = static_cast<float*>(alloc(dora_mag_grad_scratch_bytes(M, lw.secN, sizeof(T))));
        if (!scratch) return 7;
        if (dry) return 0;
        for (int j = 0; j < nmod; ++j) {
            if (!lw.mod_lora[j]) continue;
            const size_t c0 = (size_t)j * lw.secN;
            TRY(launch_dora_mag_grad<T>(static_cast<const T*>(dY) + c0, ldy, static_cast<const T*>(yout) + c0, ldyo,
                                        yres ? static_cast<const T*>(yres) + c0 : nullptr, ldres, lw.b ? lw.b + c0 : nullptr, m.theta + lw.offM[j],
                                        m.grad + lw.offM[j], M, lw.secN, lw.geglu_half, scratch, st));
        }
        return 0;
    }
    int linear_bwd(const LinW& lw, const void* x, int ldx, const float* z, const void* dY, int ldy, int M, void* dX, bool acc,
                   bool need_dx, const void* yout = nullptr, int ldyo = 0, const void* yres = nullptr, int ldres = 0) {
        float* dz = nullptr;
        float* tmpB = nullptr;
        if (lw.dora_g && lw.R) TRY(dora_mag_bwd(lw, dY, ldy, M, yout, ldyo, yres, ldres));
        bool in_kernel = false, dx_done = false;
        TRY(wgrad_linear(lw, x, ldx, dY, ldy, M));  // (full-parameter training only)
        const int nmod = (int)lw.mod_names.size();
        // where dA / dB of each adapted module go (DoRA: dB into tmpB first); valid once tmpB is decided
        float *oA[3] = {nullptr, nullptr, nullptr}, *oB[3] = {nullptr, nullptr, nullptr};
        auto grad_table = [&] {
            for (int j = 0; j < nmod; ++j) {
                if (!lw.mod_lora[j]) continue;
                oA[j] = m.grad + lw.offA[j];
                oB[j] = tmpB ? tmpB + (size_t)j * lw.secN * lw.r : m.grad + lw.offB[j];
            }
        };
        // dX (+)= dY W: the dgrad on wT (rank 32 .. 128: its second source and K are added below)
        GemmArgs g;
        if (need_dx) {
            ga_rows(g, dY, lw.n, ldy); ga_weight(g, lw.wT, M, lw.k, lw.n);
            if (acc) ga_resid(g, dX, lw.k);
            ga_out(g, dX, lw.k);
        }
        if (lw.rp) {
            // rank 32 .. 128: dz = dY (sB) is one GEMM on [R][n], dX (+)= [dY | dz] [W | A] one GEMM over K = n + R on wT, and
            // dB = dY^T z, dA = dz^T x go through lora_wgrad_hr; z and dz are T-typed
            MRISR_REQUIRE(z && lw.loraBT && m.grad && (!need_dx || lw.wT), "adapter backward state");
            T* dzt = static_cast<T*>(alloc((size_t)M * lw.R * sizeof(T)));
            const size_t sb = std::max(lora_wgrad_hr_scratch_bytes(M, lw.n, 0, lw.r, nmod, lw.secN, sizeof(T)),
                                       lora_wgrad_hr_scratch_bytes(M, lw.k, 1, lw.r, nmod, lw.secN, sizeof(T)));
            float* scratch = static_cast<float*>(alloc(sb));
            if (!dzt || !scratch) return 7;
            if (lw.dora_g) TRY(dora_b_begin(lw, &tmpB));
            GemmArgs zg;
            ga_rows(zg, dY, lw.n, ldy); ga_weight(zg, lw.loraBT, M, lw.R, lw.n); ga_out(zg, dzt, lw.R); zg.no_rp = 1;
            TRY(R::run_gemm(zg));
            if (!dry) {
                grad_table();
                TRY(launch_lora_wgrad_hr<T>(dY, ldy, z, lw.R, M, lw.n, 0, lw.r, nmod, lw.secN, oB, m.lora_scale, scratch, st, lw.geglu_half));
                TRY(launch_lora_wgrad_hr<T>(x, ldx, dzt, lw.R, M, lw.k, 1, lw.r, nmod, lw.secN, oA, 1.0f, scratch, st));
                if (tmpB) TRY(dora_b_end(lw, tmpB));
            }
            if (!need_dx) return 0;
            ga_rows2(g, dzt, lw.R, lw.R); g.K = lw.n + lw.R; g.no_rp = 1;
            return R::run_gemm(g);
        }
        if (need_dx) {
            MRISR_REQUIRE(lw.wT, "linear dgrad weights");
            // the row-panel kernel fuses LoRA only at rank 4, as in the forward: a K = 320 / 640 dgrad with R = 8 .. 16 was planned onto
            // it and then refused at launch
            if (lw.R && lw.r != 4) g.no_rp = 1;
            TRY(gemm_choose(g, sizeof(T) == 2));
            // as in the forward: dz = dY (s B) can ride along the dgrad GEMM (the <= 16 rows of s B^T as extra weight rows)
            in_kernel = sizeof(T) == 2 && g.splitk == 1 && lora_in_kernel() && gemm_tile_lora_in_kernel(g.tile, lw.r, lw.R);
        }
        if (lw.R) {
            MRISR_REQUIRE(z && lw.loraBT && lw.loraAT && m.grad, "adapter backward state");
            dz = static_cast<float*>(alloc((size_t)M * lw.R * sizeof(float)));
            const size_t sb = std::max(lora_wgrad_scratch_bytes(M, lw.n, lw.R, sizeof(T)), lora_wgrad_scratch_bytes(M, lw.k, lw.R, sizeof(T)));
            float* scratch = static_cast<float*>(alloc(sb));
            if (!dz || !scratch) return 7;
            if (lw.dora_g) TRY(dora_b_begin(lw, &tmpB));
            if (in_kernel) {  // the dgrad first: it produces dz for the A gradient
                g.lora_a = lw.loraBT; g.lora_R = lw.R; g.lora_zout = dz; ga_lora_epilogue(g, nullptr, lw.R, lw.loraAT, lw.R, INT_MAX);
                if (!dry) TRY(launch_gemm<T>(g, st));
                dx_done = true;
            }
            if (!dry) {
                if (!in_kernel) TRY(launch_lora_down<T>(dY, ldy, lw.loraBT, dz, M, lw.n, lw.R, st));
                grad_table();
                // (ff.net.0.proj: dY columns in the GEGLU interleave, gradient rows in raw order - un-interleaved by the reduce's scatter)
                TRY(launch_lora_wgrad<T>(dY, ldy, z, lw.R, M, lw.n, 0, lw.r, nmod, lw.secN, oB, m.lora_scale, scratch, st, lw.geglu_half));
                TRY(launch_lora_wgrad<T>(x, ldx, dz, lw.R, M, lw.k, 1, lw.r, nmod, lw.secN, oA, 1.0f, scratch, st));
                if (tmpB) TRY(dora_b_end(lw, tmpB));
            }
        }
        if (!need_dx || dx_done) return 0;
        if (dz) ga_lora_epilogue(g, dz, lw.R, lw.loraAT, lw.R, INT_MAX);
        return gemm_finish<T>(g, st, dry, R::arena_alloc());
    }

    struct AttnRec {
        const void* q = nullptr;   // [B*H][npad][dpad]
        const void* k = nullptr;   // [B*H][nkpad][dpad]
        const void* vt = nullptr;  // [B*H][dpad][nkpad]
        const void* P = nullptr;   // [B*H][N][nkpad] softmax probabilities (T): materialised path only
        const float* lse = nullptr;  // [B*H][npad] log-sum-exp: flash path only
        const void* out = nullptr; // attention output rows [M][C] (flash backward: D = rowsum(dO o O))
        int nk = 0, nkpad = 0;
    };
    bool flash() const { return sizeof(T) == 2 && m.cfg.flash_attention; }

    // the shared attention core (gemm_args.h), keeping what the backward needs: the log-sum-exp (flash) or P (materialised; S is released)
    int attention_t(const HeadBuf& hb, AttnRec* a, void* out_rows) {
        const AttnGeom s = R::attn_geom(hb, a->nk, a->nkpad);
        a->out = out_rows;
        if (flash()) {
            float* lse = static_cast<float*>(alloc((size_t)s.B * s.H * hb.npad * sizeof(float)));
            if (!lse) return 7;
            a->lse = lse;
            const bool fp8 = m.cfg.fp8_attention && m.cfg.fp8_train;  // fp8 forward, bf16 backward from the same log-sum-exp (straight through)
            AttnArgs fa;
            TRY(attn_flash_args(fa, s, a->q, a->k, a->vt, out_rows, lse, fp8, R::arena_alloc()));
            return attn_flash_launch(fa, fp8, dry, st);
        }
        const size_t cnt = (size_t)s.B * s.H * hb.N * a->nkpad;
        float* S;
        void* P;
        size_t mk = 0;
        if (sizeof(T) == 4) {
            S = static_cast<float*>(alloc(cnt * sizeof(float)));
            P = S;
        } else {
            P = alloc(cnt * sizeof(T));
            mk = m.arena.mark();
            S = static_cast<float*>(alloc(cnt * sizeof(float)));
        }
        if (!S || !P) return 7;
        TRY(attn_materialised<T>(s, a->q, a->k, a->vt, S, P, out_rows, dry, st, [this](GemmArgs& g) { return R::run_gemm(g); }));
        if (sizeof(T) == 2) m.arena.release(mk);
        a->P = P;
        return 0;
    }

    // dQ / dK / dV of one attention, written as token rows (head h -> columns h*hd..) at the given pointers / pitches.
    //   dV = P^T dO,  dP = dO V^T,  dS = scale * P o (dP - rowsum(dP o P)),  dQ = dS K,  dK = dS^T Q
    int attention_bwd(const HeadBuf& hb, const AttnRec& a, const void* dO_rows, T* dq, int ldq, T* dk, T* dv, int ldkv) {
        const int BH = hb.B * hb.H, N = hb.N, npad = hb.npad, dpad = hb.dpad, nk = a.nk, nkpad = a.nkpad;
        const float scale = 1.0f / sqrtf((float)hb.hd);
        const size_t qsz = (size_t)BH * npad * dpad, ksz = (size_t)BH * nkpad * dpad, psz = (size_t)BH * N * nkpad;
        if (flash()) {
            // P recomputed from the log-sum-exp inside the kernels; only [tokens x head dim] operands are staged
            void* doh = alloc(qsz * sizeof(T));
            float* dsum = static_cast<float*>(alloc((size_t)BH * npad * sizeof(float)));
            void* V = alloc(ksz * sizeof(T));
            void* Kt = alloc(ksz * sizeof(T));
            void* Qt = dk ? alloc(qsz * sizeof(T)) : nullptr;
            void* doht = dk ? alloc(qsz * sizeof(T)) : nullptr;
            if (!doh || !dsum || !V || !Kt || (dk && (!Qt || !doht))) return 7;
            TRY(zero(doh, qsz * sizeof(T)));
            TRY(zero(dsum, (size_t)BH * npad * sizeof(float)));
            if (dry) return 0;
            TRY(launch_attention_bwd_prep(dO_rows, a.out, doh, dsum, hb.B, N, hb.H, hb.hd, npad, dpad, st));
            TRY(launch_transpose<T>(a.vt, V, dpad, nkpad, nkpad, dpad, (long long)dpad * nkpad, (long long)nkpad * dpad, BH, dpad, st));
            TRY(launch_transpose<T>(a.k, Kt, nkpad, dpad, dpad, nkpad, (long long)nkpad * dpad, (long long)dpad * nkpad, BH, nkpad, st));
            if (dk) {
                TRY(launch_transpose<T>(a.q, Qt, npad, dpad, dpad, npad, (long long)npad * dpad, (long long)dpad * npad, BH, npad, st));
                TRY(launch_transpose<T>(doh, doht, npad, dpad, dpad, npad, (long long)npad * dpad, (long long)dpad * npad, BH, npad, st));
            }
            AttnBwdArgs g;
            g.q = a.q; g.k = a.k; g.v = V; g.doh = doh; g.qt = Qt; g.kt = Kt; g.doht = doht; g.lse = a.lse; g.dsum = dsum;
            g.dq = dq; g.ldq = ldq; g.dk = dk; g.dv = dv; g.ldkv = ldkv;
            g.B = hb.B; g.H = hb.H; g.nq = N; g.nk = nk; g.npad = npad; g.nkpad = nkpad; g.hd = hb.hd; g.dpad = dpad; g.scale = scale;
            return launch_attention_bwd_bf16(g, st);
        }
        T* dOh = static_cast<T*>(alloc(qsz * sizeof(T)));
        T* V = static_cast<T*>(alloc(ksz * sizeof(T)));
        float* dP = static_cast<float*>(alloc(psz * sizeof(float)));
        T* dS = static_cast<T*>(alloc(psz * sizeof(T)));
        T* Kt = static_cast<T*>(alloc(ksz * sizeof(T)));
        if (!dOh || !V || !dP || !dS || !Kt) return 7;
        TRY(zero(dOh, qsz * sizeof(T)));
        if (!dry) {
            TRY(launch_rows_to_heads<T>(dO_rows, hb.H * hb.hd, 0, dOh, hb.B, N, hb.H, hb.hd, npad, dpad, st));
            TRY(launch_transpose<T>(a.vt, V, dpad, nkpad, nkpad, dpad, (long long)dpad * nkpad, (long long)nkpad * dpad, BH, dpad, st));
            TRY(launch_transpose<T>(a.k, Kt, nkpad, dpad, dpad, nkpad, (long long)nkpad * dpad, (long long)dpad * nkpad, BH, nkpad, st));
        }
        {   // dP = dOh V^T
            GemmArgs g;
            ga_rows(g, dOh, dpad, dpad); ga_weight(g, V, N, nkpad, dpad);
            ga_batch(g, BH, (long long)npad * dpad, (long long)nkpad * dpad, (long long)N * nkpad); ga_out_f32(g, dP, nkpad);
            TRY(R::run_gemm(g));
        }
        if (!dry) TRY(launch_softmax_bwd<T>(a.P, dP, dS, nkpad, (long long)BH * N, nk, scale, st));
        {   // dQ = dS K  (W operand = K^T)
            GemmArgs g;
            ga_rows(g, dS, nkpad, nkpad); ga_weight(g, Kt, N, hb.hd, nkpad);
            ga_batch_heads(g, BH, (long long)N * nkpad, (long long)dpad * nkpad, hb.H, (long long)N * ldq, hb.hd); ga_out(g, dq, ldq);
            TRY(R::run_gemm(g));
        }
        if (!dk) return 0;
        T* At = static_cast<T*>(alloc((size_t)BH * nkpad * npad * sizeof(T)));  // dS^T, then P^T
        T* Wt = static_cast<T*>(alloc(qsz * sizeof(T)));                        // Q^T, then dOh^T
        if (!At || !Wt) return 7;
        TRY(zero(At, (size_t)BH * nkpad * npad * sizeof(T)));  // token pads N..npad stay zero through both uses
        auto kv_grad = [&](const void* a_src, const void* w_src, T* out) -> int {
            if (!dry) {
                TRY(launch_transpose<T>(a_src, At, N, nkpad, nkpad, npad, (long long)N * nkpad, (long long)nkpad * npad, BH, N, st));
                TRY(launch_transpose<T>(w_src, Wt, npad, dpad, dpad, npad, (long long)npad * dpad, (long long)dpad * npad, BH, npad, st));
            }
            GemmArgs g;
            ga_rows(g, At, npad, npad); ga_weight(g, Wt, nk, hb.hd, npad);
            ga_batch_heads(g, BH, (long long)nkpad * npad, (long long)dpad * npad, hb.H, (long long)nk * ldkv, hb.hd); ga_out(g, out, ldkv);
            return R::run_gemm(g);
        };
        TRY(kv_grad(dS, a.q, dk));
        TRY(kv_grad(a.P, dOh, dv));
        return 0;
    }

    // ---------------------------------------------------------------------------------------------
    // ResnetBlock2D
    // ---------------------------------------------------------------------------------------------
    // backward of the adapter of one 3x3 conv, y = conv(x, W) + s B conv3x3(x, A):  dz = dY (s B);  dB = s dY^T z and dA = the weight gradient of
    // the r-channel conv (dz as its dY) into m.grad;  dX += the transposed conv of dz (dX holds the base conv's dgrad already; null: not needed)
    int conv_lora_bwd(const ConvW& cw, const Act& x, const float* z, const void* dY, void* dX) {
        const int M = (int)x.rows(), R = cw.r;
        MRISR_REQUIRE(z && cw.loraBT && cw.loraA && m.grad && cw.offLA >= 0 && cw.offLB >= 0 && x.C == cw.cin, "conv adapter backward state");
        const size_t mk = m.arena.mark();
        float* dz = static_cast<float*>(alloc((size_t)M * R * sizeof(float)));
        float* scratch = static_cast<float*>(alloc(lora_wgrad_scratch_bytes(M, cw.cout, R, sizeof(T))));
        void* dzT = sizeof(T) == 4 ? static_cast<void*>(dz) : alloc((size_t)M * R * sizeof(T));
        if (!dz || !scratch || !dzT) return 7;
        if (!dry) {
            TRY(launch_lora_down<T>(dY, cw.cout, cw.loraBT, dz, M, cw.cout, R, st));
            float* oB[3] = {m.grad + cw.offLB, nullptr, nullptr};
            TRY(launch_lora_wgrad<T>(dY, cw.cout, z, R, M, cw.cout, 0, R, 1, cw.cout, oB, m.lora_scale, scratch, st));
            if (sizeof(T) == 2) TRY(launch_cast_rows<T>(dz, dzT, (long long)M * R, st));
        }
        TRY(wgrad(x.p, x.B, x.H, x.W, x.C, dzT, R, 0, x.H, x.W, R, 3, 1, m.grad + cw.offLA, nullptr, R, x.C));
        if (dX && !dry) TRY(launch_conv_lora_dgrad<T>(dz, cw.loraA, cw.loraAd, dX, x.B, x.H, x.W, x.C, R, 1, st));
        m.arena.release(mk);
        return 0;
    }

    int resnet_t(const ResW& r, const Act& x, const Act* x1, Act* out) {
        Act o = new_act(x.B, x.H, x.W, r.cout);
        if (!o.p) return 7;
        typename R::ResTape ft;
        TRY(R::resnet_literal(r, x, x1, o, &ft));
        const Act xn = ft.xn, h = ft.h, hn = ft.hn;
        float *p1 = ft.p1, *p2 = ft.p2, *z1 = ft.z1, *z2 = ft.z2;
        const int ns1 = ft.ns1, ns2 = ft.ns2;
        *out = o;
        // an adapter makes the block live even when its input is not (the first resnet after conv_in): weight gradients only, then
        const bool x_live = is_live(x) || (x1 && is_live(*x1));
        if (!x_live && !r.c1.r && !r.c2.r) return 0;  // nothing trainable upstream or inside: the block has no backward
        live.insert(o.p);
        const bool has_x1 = x1 != nullptr;
        const Act x1v = x1 ? *x1 : Act();
        const ResW* rp = &r;
        tape.push_back([=]() -> int {
            const ResW& rr = *rp;
            auto it = slots.find(o.p);
            MRISR_REQUIRE(it != slots.end() && it->second.written, "resnet output has no gradient");
            void* dO = it->second.g;
            Slot* s0 = x_live ? &slot(x) : nullptr;
            Slot* s1 = x_live && has_x1 ? &slot(x1v) : nullptr;
            const size_t mk = m.arena.mark();
            Act dOa = o; dOa.p = dO;
            if (!x_live && !rr.c1.r) {  // only conv2 is adapted and nothing upstream wants dX: its weight gradients alone
                TRY(conv_lora_bwd(rr.c2, hn, z2, dO, nullptr));
                m.arena.release(mk);
                return 0;
            }
            Act dhn = new_act(o.B, o.H, o.W, rr.cout), dh = new_act(o.B, o.H, o.W, rr.cout);
            if (!dhn.p || !dh.p) return 7;
            TRY(wgrad_conv(hn, dOa, rr.c2, 1));
            TRY(conv_dgrad(dOa, rr.c2, 0, dhn.p, false));
            if (rr.c2.r) TRY(conv_lora_bwd(rr.c2, hn, z2, dO, dhn.p));
            TRY(gn_affine(h, dhn.p, rr.n2, true, m.cfg.norm_eps, p2, ns2));
            TRY(gn_bwd(h, nullptr, rr.n2, true, m.cfg.norm_eps, p2, ns2, dhn.p, dh.p, false, nullptr, false));
            if (full() && m.d_tproj && !dry)  // h = conv1(.) + time_emb_proj(silu(emb))[:, :, None, None]: its gradient is the per-image sum of dh
                TRY(launch_rowvec_grad<T>(dh.p, m.d_tproj, m.tproj_total, rr.temb_off, o.B, o.H * o.W, rr.cout, m.t_scalar, st));
            TRY(wgrad_conv(xn, dh, rr.c1, 1));
            if (full() && rr.has_sc) {
                MRISR_REQUIRE(!has_x1, "full-parameter training: single-source shortcut");
                TRY(wgrad_linear(rr.sc, x.p, x.C, dO, rr.cout, (int)x.rows()));
            }
            if (!x_live) {  // conv1's adapter gradients and nothing beyond the block
                TRY(conv_lora_bwd(rr.c1, xn, z1, dh.p, nullptr));
                m.arena.release(mk);
                return 0;
            }
            Act dxn = new_act(o.B, o.H, o.W, rr.cin);
            if (!dxn.p) return 7;
            TRY(conv_dgrad(dh, rr.c1, 0, dxn.p, false));
            if (rr.c1.r) TRY(conv_lora_bwd(rr.c1, xn, z1, dh.p, dxn.p));
            if (!has_x1) TRY(gn_affine(x, dxn.p, rr.n1, true, m.cfg.norm_eps, p1, ns1));
            TRY(gn_bwd(x, has_x1 ? &x1v : nullptr, rr.n1, true, m.cfg.norm_eps, p1, ns1, dxn.p, s0->g, s0->written,
                       s1 ? s1->g : nullptr, s1 ? s1->written : false));
            s0->written = true;
            if (s1) s1->written = true;
            if (rr.has_sc) {
                // 1x1 shortcut over the concatenated input: one dgrad GEMM per source, accumulated in place
                const T* wT = static_cast<const T*>(rr.sc.wT);
                MRISR_REQUIRE(wT, "shortcut dgrad weights");
                auto source_dgrad = [&](const T* w, int c, void* gx) -> int {
                    GemmArgs g;
                    ga_rows(g, dO, rr.cout, rr.cout); ga_weight(g, w, (int)x.rows(), c, rr.cout); ga_resid(g, gx, c); ga_out(g, gx, c);
                    return R::run_gemm(g);
                };
                TRY(source_dgrad(wT, x.C, s0->g));
                if (s1) TRY(source_dgrad(wT + (size_t)x.C * rr.cout, x1v.C, s1->g));
            } else if (!dry) {
                TRY(launch_add_inplace<T>(s0->g, dO, (long long)x.numel(), st));
            }
            m.arena.release(mk);
            return 0;
        });
        return 0;
    }

    // ---------------------------------------------------------------------------------------------
    // Transformer2DModel / BasicTransformerBlock
    // ---------------------------------------------------------------------------------------------
    int transformer_t(XfW& xw, const Act& x, Act* out) {
        const int C = xw.C, M = (int)x.rows();
        const HeadBuf& hb = m.head_buf(x.H * x.W, C);
        const int Bc = m.ws_B * m.ctx_len;
        Act o = new_act(x.B, x.H, x.W, C);
        if (!o.p) return 7;
        Act xn;
        float* gp = nullptr;
        int gns = 1;
        TRY(R::gn(x, nullptr, xw.norm, false, 1e-6f, &xn, &gp, &gns));
        auto rows = [&](int c) { return static_cast<T*>(alloc((size_t)M * c * sizeof(T))); };
        T *t0 = rows(C), *n1 = rows(C), *ao1 = rows(C), *t1 = rows(C), *n2 = rows(C), *ao2 = rows(C), *t2 = rows(C), *n3 = rows(C);
        T *ffpre = rows(8 * C), *ff = rows(4 * C), *t3 = rows(C);
        const size_t hsz = (size_t)hb.B * hb.H * hb.npad * hb.dpad * sizeof(T);
        void *q1 = alloc(hsz), *k1 = alloc(hsz), *vt1 = alloc(hsz), *q2 = alloc(hsz);
        if (!t3 || !q2) return 7;
        TRY(zero(q1, hsz)); TRY(zero(k1, hsz)); TRY(zero(vt1, hsz)); TRY(zero(q2, hsz));
        float *z_pi = nullptr, *z_qkv = nullptr, *z_o1 = nullptr, *z_q2 = nullptr, *z_o2 = nullptr, *z_f1 = nullptr, *z_f2 = nullptr, *z_po = nullptr;
        TRY(R::linear(xn.p, M, C, xw.proj_in, ACT_NONE, nullptr, 0, nullptr, t0, C, &z_pi));
        TRY(R::layernorm(t0, xw.ln1, M, C, n1));
        {
            GemmArgs g;
            R::heads_args(&g, hb, q1, 0, k1, 0, vt1, 1, hb.N, hb.npad);
            TRY(R::linear(n1, M, C, xw.qkv, ACT_NONE, nullptr, 0, &g, nullptr, 0, &z_qkv));
        }
        // DoRA: the magnitude's gradient reads a projection's output as rows; q / k / v survive head-major only, so a DoRA projection runs
        // once more into rows (and proj_out's output is copied: later stages may add into it in place)
        T *y_qkv = nullptr, *y_q2 = nullptr, *y_po = nullptr;
        if (xw.qkv.dora_g) {
            y_qkv = rows(3 * C);
            if (!y_qkv) return 7;
            TRY(R::linear(n1, M, C, xw.qkv, ACT_NONE, nullptr, 0, nullptr, y_qkv, 3 * C));
        }
        AttnRec a1;
        a1.q = q1; a1.k = k1; a1.vt = vt1; a1.nk = hb.N; a1.nkpad = hb.npad;
        TRY(attention_t(hb, &a1, ao1));
        TRY(R::linear(ao1, M, C, xw.out1, ACT_NONE, t0, C, nullptr, t1, C, &z_o1));
        TRY(R::layernorm(t1, xw.ln2, M, C, n2));
        {
            GemmArgs g;
            R::heads_args(&g, hb, q2, 0, nullptr, 0, nullptr, 0, hb.N, hb.npad);
            TRY(R::linear(n2, M, C, xw.q2, ACT_NONE, nullptr, 0, &g, nullptr, 0, &z_q2));
        }
        if (xw.q2.dora_g) {
            y_q2 = rows(C);
            if (!y_q2) return 7;
            TRY(R::linear(n2, M, C, xw.q2, ACT_NONE, nullptr, 0, nullptr, y_q2, C));
        }
        AttnRec a2;
        a2.q = q2; a2.k = xw.kc; a2.vt = xw.vtc; a2.nk = m.ctx_len; a2.nkpad = m.ctx_pad;
        TRY(attention_t(hb, &a2, ao2));
        TRY(R::linear(ao2, M, C, xw.out2, ACT_NONE, t1, C, nullptr, t2, C, &z_o2));
        TRY(R::layernorm(t2, xw.ln3, M, C, n3));
        TRY(R::linear(n3, M, C, xw.ff1, ACT_NONE, nullptr, 0, nullptr, ffpre, 8 * C, &z_f1));
        if (!dry) TRY(launch_geglu_fwd<T>(ffpre, ff, M, 4 * C, st));
        TRY(R::linear(ff, M, 4 * C, xw.ff2, ACT_NONE, t2, C, nullptr, t3, C, &z_f2));
        TRY(R::linear(t3, M, C, xw.proj_out, ACT_NONE, x.p, C, nullptr, o.p, C, &z_po));
        if (xw.proj_out.dora_g) {
            y_po = rows(C);
            if (!y_po) return 7;
            if (!dry) MRISR_CHECK_HIP(hipMemcpyAsync(y_po, o.p, (size_t)M * C * sizeof(T), hipMemcpyDeviceToDevice, st));
        }
        *out = o;
        const bool x_live = is_live(x);
        if (!x_live && !has_lora(xw) && !full()) return 0;
        live.insert(o.p);
        const XfW* xp = &xw;
        const HeadBuf hbv = hb;
        float* zkv = z_kv.count(&xw) ? z_kv[&xw] : nullptr;
        const void* ykv = y_kv.count(&xw) ? y_kv[&xw] : nullptr;
        tape.push_back([=]() -> int {
            const XfW& w = *xp;
            auto it = slots.find(o.p);
            MRISR_REQUIRE(it != slots.end() && it->second.written, "transformer output has no gradient");
            void* dO = it->second.g;
            Slot* sx = x_live ? &slot(x) : nullptr;
            const size_t mk = m.arena.mark();
            auto brows = [&](size_t r, int c) { return static_cast<T*>(alloc(r * c * sizeof(T))); };
            T *dt = brows(M, C), *dn = brows(M, C), *dao = brows(M, C), *dq = brows(M, C);
            T *dff = brows(M, 4 * C), *dpre = brows(M, 8 * C), *dqkv = brows(M, 3 * C);
            const bool want_kv = w.kv2.R || full();
            T* dkv = want_kv ? brows(Bc, 2 * C) : nullptr;
            if (!dt || !dn || !dao || !dq || !dff || !dpre || !dqkv || (want_kv && !dkv)) return 7;
            // o = proj_out(t3) + x
            TRY(linear_bwd(w.proj_out, t3, C, z_po, dO, C, M, dt, false, true, y_po, C, x.p, C));
            // t3 = t2 + ff2(geglu(ff1(LN3(t2))))
            TRY(linear_bwd(w.ff2, ff, 4 * C, z_f2, dt, C, M, dff, false, true, t3, C, t2, C));
            if (!dry) TRY(launch_geglu_bwd<T>(ffpre, dff, dpre, M, 4 * C, st));
            TRY(linear_bwd(w.ff1, n3, C, z_f1, dpre, 8 * C, M, dn, false, true, ffpre, 8 * C));
            TRY(ln_affine(t2, dn, w.ln3, M, C));
            if (!dry) TRY(launch_layernorm_bwd<T>(t2, dn, dt, w.ln3.g, M, C, 1e-5f, 1, st));
            // t2 = t1 + out2(attn(q2(LN2(t1)), K_ctx, V_ctx))
            TRY(linear_bwd(w.out2, ao2, C, z_o2, dt, C, M, dao, false, true, t2, C, t1, C));
            TRY(attention_bwd(hbv, a2, dao, dq, C, dkv, dkv ? dkv + C : nullptr, 2 * C));
            if (dkv) TRY(linear_bwd(w.kv2, m.ctx_rows, m.cfg.cross_attention_dim, zkv, dkv, 2 * C, Bc, nullptr, false, false, ykv, 2 * C));
            TRY(linear_bwd(w.q2, n2, C, z_q2, dq, C, M, dn, false, true, y_q2, C));
            TRY(ln_affine(t1, dn, w.ln2, M, C));
            if (!dry) TRY(launch_layernorm_bwd<T>(t1, dn, dt, w.ln2.g, M, C, 1e-5f, 1, st));
            // t1 = t0 + out1(attn(qkv(LN1(t0))))
            TRY(linear_bwd(w.out1, ao1, C, z_o1, dt, C, M, dao, false, true, t1, C, t0, C));
            TRY(attention_bwd(hbv, a1, dao, dqkv, 3 * C, dqkv + C, dqkv + 2 * C, 3 * C));
            TRY(linear_bwd(w.qkv, n1, C, z_qkv, dqkv, 3 * C, M, dn, false, true, y_qkv, 3 * C));
            TRY(ln_affine(t0, dn, w.ln1, M, C));
            if (!dry) TRY(launch_layernorm_bwd<T>(t0, dn, dt, w.ln1.g, M, C, 1e-5f, 1, st));
            // t0 = proj_in(GN(x))
            if (sx) {
                TRY(linear_bwd(w.proj_in, xn.p, C, z_pi, dt, C, M, dn, false, true, t0, C));
                TRY(gn_affine(x, dn, w.norm, false, 1e-6f, gp, gns));
                TRY(gn_bwd(x, nullptr, w.norm, false, 1e-6f, gp, gns, dn, sx->g, sx->written, nullptr, false));
                sx->written = true;
                if (!dry) TRY(launch_add_inplace<T>(sx->g, dO, (long long)x.numel(), st));
            } else if (w.proj_in.R) {
                TRY(linear_bwd(w.proj_in, xn.p, C, z_pi, dt, C, M, nullptr, false, false, t0, C));
            }
            m.arena.release(mk);
            return 0;
        });
        return 0;
    }

    // ---------------------------------------------------------------------------------------------
    // whole network
    // ---------------------------------------------------------------------------------------------
    int set_context_t(const mrisr_tensor& ehs) {
        MRISR_REQUIRE(ehs.ndim == 3 && ehs.shape[2] == m.cfg.cross_attention_dim, "encoder_hidden_states shape");
        MRISR_REQUIRE((int)ehs.shape[0] == m.ws_B && (int)ehs.shape[1] == m.ctx_len, "context shape vs planned workspace");
        if (!dry) TRY(launch_nchw_to_nhwc<T>(ehs.data, ehs.dtype, m.ctx_rows, m.ws_B * m.ctx_len, m.cfg.cross_attention_dim, 1, 1, st));
        int rc = 0;
        for_each_xf(m, [&](XfW& x) {
            if (rc) return;
            const HeadBuf& hb = m.head_buf_for_C(x.C);
            GemmArgs g;
            R::heads_args(&g, hb, x.kc, 0, x.vtc, 1, nullptr, 0, m.ctx_len, m.ctx_pad);
            float* z = nullptr;
            rc = R::linear(m.ctx_rows, m.ws_B * m.ctx_len, m.cfg.cross_attention_dim, x.kv2, ACT_NONE, nullptr, 0, &g, nullptr, 0, &z);
            z_kv[&x] = z;
            if (!rc && x.kv2.dora_g) {
                void* y = alloc((size_t)m.ws_B * m.ctx_len * x.kv2.n * sizeof(T));
                rc = y ? R::linear(m.ctx_rows, m.ws_B * m.ctx_len, m.cfg.cross_attention_dim, x.kv2, ACT_NONE, nullptr, 0, nullptr, y, x.kv2.n) : 7;
                y_kv[&x] = y;
            }
        });
        m.ctx_valid = false;  // the cache belongs to this step's adapters only
        return rc;
    }

    // x = x + feature (T2I-Adapter): when the backward reaches this point every consumer of x has contributed, so d(x) is
    // also d(feature); hand it to the caller's tensor (mrisr_train_set_intrablock_grads) for the adapter's own backward
    int export_feature_grad(const Act& x, int ib) {
        if (ib >= (int)m.d_intra.size() || !m.d_intra[ib].data) return 0;
        // a frozen UNet (no LoRA upstream): the feature itself is the trainable input, so x carries a gradient from here on
        if (!is_live(x)) live.insert(x.p);
        const mrisr_tensor out = m.d_intra[ib];
        tape.push_back([=]() -> int {
            auto it = slots.find(x.p);
            MRISR_REQUIRE(it != slots.end() && it->second.written, "feature position has no gradient");
            Act gx = x;
            gx.p = it->second.g;
            return R::export_act(gx, out, 1.0f);
        });
        return 0;
    }

    // y = copy(x) + r (a ControlNet residual, diffusers: `down_block_res_sample + down_block_additional_residual`, out of place - the
    // encoder's own flow and its saved activations keep the un-added tensor): d(r) = d(y) -> the caller's tensor; d(x) += d(y)
    int add_residual_t(const Act& x, const mrisr_tensor& r, const mrisr_tensor* d_out, Act* y) {
        *y = new_act(x.B, x.H, x.W, x.C);
        if (!y->p) return 7;
        if (!dry) MRISR_CHECK_HIP(hipMemcpyAsync(y->p, x.p, x.numel() * sizeof(T), hipMemcpyDeviceToDevice, st));
        TRY(R::add_external(*y, r));
        live.insert(y->p);  // trainable upstream: the ControlNet
        const Act yy = *y;
        const bool x_live = is_live(x);
        const bool want = d_out && d_out->data;
        const mrisr_tensor out = want ? *d_out : mrisr_tensor{};
        tape.push_back([=]() -> int {
            auto it = slots.find(yy.p);
            MRISR_REQUIRE(it != slots.end() && it->second.written, "residual position has no gradient");
            Act gy = yy;
            gy.p = it->second.g;
            if (want) TRY(R::export_act(gy, out, 1.0f));
            if (x_live) {
                Slot& sx = slot(x);
                if (!dry) {
                    if (sx.written) TRY(launch_add_inplace<T>(sx.g, it->second.g, (long long)x.numel(), st));
                    else MRISR_CHECK_HIP(hipMemcpyAsync(sx.g, it->second.g, x.numel() * sizeof(T), hipMemcpyDeviceToDevice, st));
                }
                sx.written = true;
            }
            return 0;
        });
        return 0;
    }

    // dst.grad (+)= src.grad   (y = copy(x) [+ constant])
    int pass_grad(const Act& y, const Act& x) {
        if (!is_live(x)) return 0;
        live.insert(y.p);
        tape.push_back([=]() -> int {
            auto it = slots.find(y.p);
            MRISR_REQUIRE(it != slots.end() && it->second.written, "copy has no gradient");
            Slot& sx = slot(x);
            if (!dry) {
                if (sx.written) TRY(launch_add_inplace<T>(sx.g, it->second.g, (long long)x.numel(), st));
                else MRISR_CHECK_HIP(hipMemcpyAsync(sx.g, it->second.g, x.numel() * sizeof(T), hipMemcpyDeviceToDevice, st));
            }
            sx.written = true;
            return 0;
        });
        return 0;
    }

    // ---------------------------------------------------------------------------------------------
    // ControlNet with every parameter trainable (full-parameter mode).  Forward = Runner::controlnet_forward's sequence, recorded;
    // the backward is seeded with d(loss)/d(residual k) - what the UNet's step exported (mrisr_train_set_controlnet_residuals).
    // ---------------------------------------------------------------------------------------------
    // ControlNet condition embedding (App. A.6: conv_in, six blocks, conv_out; SiLU after all but the last) with the pre-activations kept
    // - the inference path fuses the SiLU into the conv epilogue and caches only the result.  Layers 1.. run zero-padded to 64-channel
    // multiples (model.hip conv_padded): gradients flow through the padded banks, the raw tensors receive their sub-blocks.
    std::vector<Act> ce_in, ce_pre;
    int set_cond_t(const mrisr_tensor& cond) {
        Act e, y;
        TRY(R::import_act(cond, &e, false));
        ce_in.clear();
        ce_pre.clear();
        for (size_t k = 0; k < m.ce.size(); ++k) {
            const bool last = k + 1 == m.ce.size();
            constexpr int KQ = 128 / (int)sizeof(T);
            ce_in.push_back(e);
            if (e.C % KQ == 0 && m.ce[k].cout % 4 == 0) TRY(R::conv3(e, nullptr, m.ce[k], m.ce_stride[k], 0, nullptr, 0, 1, nullptr, ACT_NONE, &y));
            else TRY(R::direct(e, m.ce[k], m.ce_stride[k], ACT_NONE, nullptr, &y));
            ce_pre.push_back(y);
            if (!last) {
                Act a = new_act(y.B, y.H, y.W, y.C);
                if (!a.p) return 7;
                if (!dry) TRY(launch_silu_fwd<T>(y.p, a.p, (long long)y.numel(), st));
                e = a;
            } else {
                e = y;
            }
        }
        MRISR_REQUIRE(e.numel() * sizeof(T) <= m.cond_emb_bytes, "condition embedding larger than planned");
        if (!dry) MRISR_CHECK_HIP(hipMemcpyAsync(m.cond_emb, e.p, e.numel() * sizeof(T), hipMemcpyDeviceToDevice, st));
        m.cond_valid = false;  // (the cache holds THIS step's weights only)
        return 0;
    }
    int set_cond_bwd(const Act& d_ce) {  // d_ce: gradient with respect to the embedding = the gradient of conv_in's output
        const size_t mk = m.arena.mark();
        Act dcur = d_ce;
        for (size_t kk = m.ce.size(); kk-- > 0;) {
            const ConvW& cw = m.ce[kk];
            const bool last = kk + 1 == m.ce.size();
            const Act& pre = ce_pre[kk];
            const Act& xin = ce_in[kk];
            Act dpre = dcur;
            if (!last) {
                dpre = new_act(pre.B, pre.H, pre.W, pre.C);
                if (!dpre.p) return 7;
                if (!dry) TRY(launch_silu_bwd<T>(dcur.p, pre.p, dpre.p, (long long)pre.numel(), st));
            }
            const RawParam* w = m.find(cw.name + ".weight");
            MRISR_REQUIRE(w && dpre.C == cw.cout && xin.C == cw.cin, "condition-embedding gradient: operands");
            TRY(wgrad(xin.p, xin.B, xin.H, xin.W, xin.C, dpre.p, dpre.C, 0, dpre.H, dpre.W, dpre.C, cw.ks, m.ce_stride[kk], gptr(cw.name + ".weight"),
                      gptr(cw.name + ".bias"), (int)w->shape[0], (int)w->shape[1]));
            if (kk > 0) {
                Act dx = new_act(xin.B, xin.H, xin.W, xin.C);
                if (!dx.p) return 7;
                TRY(conv_dgrad(dpre, cw, m.ce_stride[kk] == 2 ? 1 : 0, dx.p, false));
                dcur = dx;
            }
        }
        m.arena.release(mk);
        return 0;
    }

    std::vector<Act> cn_skips;
    Act cn_x;  // mid-block output
    int cn_B = 0;
    int cn_forward(const mrisr_tensor& sample, const long long* t_dev, int t_scalar, const mrisr_tensor& ehs, const mrisr_tensor& cond, float scale,
                   mrisr_tensor* down_out, int n_down, mrisr_tensor* mid_out) {
        m.arena.reset();
        const int B = (int)sample.shape[0];
        TRY(set_context_t(ehs));
        TRY(set_cond_t(cond));
        TRY(R::time_embed(t_dev, t_scalar, B));
        {
            const size_t nb = (size_t)(t_scalar ? 1 : B) * m.tproj_total * sizeof(float);
            m.d_tproj = static_cast<float*>(alloc(nb));
            TRY(zero(m.d_tproj, nb));
        }
        cn_B = B;
        Act s, x;
        TRY(R::import_act(sample, &s, false));
        Act ce;
        ce.p = m.cond_emb; ce.B = B; ce.H = s.H; ce.W = s.W; ce.C = m.cfg.block_out_channels[0];
        TRY(R::direct(s, m.conv_in, 1, ACT_NONE, &ce, &x));
        live.insert(x.p);
        {   // conv_in's own weights (4 input channels: the generic pixel-contraction path)
            const Act sv = s, xv = x;
            tape.push_back([=]() -> int {
                auto it = slots.find(xv.p);
                MRISR_REQUIRE(it != slots.end() && it->second.written, "conv_in output has no gradient");
                Act dy = xv; dy.p = it->second.g;
                TRY(wgrad_conv(sv, dy, m.conv_in, 1));
                return set_cond_bwd(dy);  // x = conv_in(sample) + embedding: the embedding's gradient is the same tensor
            });
        }
        cn_skips.clear();
        cn_skips.push_back(x);
        for (int i = 0; i < m.cfg.num_levels; ++i) {
            Level& lv = m.down[i];
            const bool has_attn = !lv.xf.empty();
            for (size_t j = 0; j < lv.res.size(); ++j) {
                Act y;
                TRY(resnet_t(lv.res[j], x, nullptr, &y));
                x = y;
                if (has_attn) {
                    TRY(transformer_t(lv.xf[j], x, &y));
                    x = y;
                }
                cn_skips.push_back(x);
            }
            if (lv.has_down) {
                Act y;
                TRY(R::conv3(x, nullptr, lv.down, 2, 0, nullptr, 0, 1, nullptr, ACT_NONE, &y));
                live.insert(y.p);
                const ConvW* cw = &lv.down;
                const Act xin = x;
                tape.push_back([=]() -> int {
                    auto it = slots.find(y.p);
                    MRISR_REQUIRE(it != slots.end() && it->second.written, "downsample output has no gradient");
                    Slot& sx = slot(xin);
                    Act dy = y; dy.p = it->second.g;
                    TRY(wgrad_conv(xin, dy, *cw, 2));
                    TRY(conv_dgrad(dy, *cw, 1, sx.g, sx.written));
                    sx.written = true;
                    return 0;
                });
                x = y;
                cn_skips.push_back(x);
            }
        }
        {
            Act y;
            TRY(resnet_t(m.mid_r0, x, nullptr, &y));
            x = y;
            TRY(transformer_t(m.mid_xf, x, &y));
            x = y;
            TRY(resnet_t(m.mid_r1, x, nullptr, &y));
            x = y;
        }
        cn_x = x;
        MRISR_REQUIRE(n_down == (int)cn_skips.size(), "ControlNet output count");
        for (int k = 0; k <= n_down; ++k) {  // the zero convs (k == n_down: the mid block's)
            const Act& a = k < n_down ? cn_skips[k] : cn_x;
            const LinW& zw = k < n_down ? m.cn_down[k] : m.cn_mid;
            Act o = new_act(a.B, a.H, a.W, a.C);
            if (!o.p) return 7;
            TRY(R::linear(a.p, (int)a.rows(), a.C, zw, ACT_NONE, nullptr, 0, nullptr, o.p, o.C));
            mrisr_tensor* dst = k < n_down ? &down_out[k] : mid_out;
            if (dst && dst->data) TRY(R::export_act(o, *dst, scale));
        }
        return 0;
    }
    int cn_backward(const mrisr_tensor* d_down, int n_down, const mrisr_tensor* d_mid, float scale) {
        MRISR_REQUIRE(n_down == (int)cn_skips.size() && d_mid, "one gradient per ControlNet residual");
        for (int k = n_down; k >= 0; --k) {
            const Act& a = k < n_down ? cn_skips[k] : cn_x;
            const LinW& zw = k < n_down ? m.cn_down[k] : m.cn_mid;
            const mrisr_tensor& src = k < n_down ? d_down[k] : *d_mid;
            MRISR_REQUIRE(src.ndim == 4 && src.shape[0] == a.B && src.shape[1] == a.C && src.shape[2] == a.H && src.shape[3] == a.W, "residual gradient shape");
            Slot& sa = slot(a);  // (allocates the gradient buffer on first use: BEFORE the mark, it must outlive this scope)
            const size_t mk = m.arena.mark();
            Act dy;
            TRY(R::import_act(src, &dy, true));
            if (scale != 1.0f && !dry) TRY(launch_scale_inplace<T>(dy.p, scale, (long long)dy.numel(), st));
            TRY(linear_bwd(zw, a.p, a.C, nullptr, dy.p, a.C, (int)a.rows(), sa.g, sa.written, true));
            sa.written = true;
            m.arena.release(mk);
        }
        for (size_t i = tape.size(); i-- > 0;) TRY(tape[i]());
        return time_embed_bwd(cn_B);
    }

    int step(const mrisr_tensor& sample, const long long* t_dev, int t_scalar, const mrisr_tensor& ehs, const mrisr_tensor* intrablock,
             int n_intra, const mrisr_tensor& target, float* loss_dev, const mrisr_tensor* pred_out) {
        m.arena.reset();
        const int B = (int)sample.shape[0];
        TRY(set_context_t(ehs));
        TRY(R::time_embed(t_dev, t_scalar, B));
        Act s, x;
        TRY(R::import_act(sample, &s, false));
        TRY(R::direct(s, m.conv_in, 1, ACT_NONE, nullptr, &x));
        // ---- encoder ----
        std::vector<Act> skips;
        skips.push_back(x);
        int ib = 0;
        for (int i = 0; i < m.cfg.num_levels; ++i) {
            Level& lv = m.down[i];
            const bool has_attn = !lv.xf.empty();
            for (size_t j = 0; j < lv.res.size(); ++j) {
                Act y;
                TRY(resnet_t(lv.res[j], x, nullptr, &y));
                x = y;
                if (has_attn) {
                    TRY(transformer_t(lv.xf[j], x, &y));
                    x = y;
                    if (j + 1 == lv.res.size() && ib < n_intra) {
                        TRY(R::add_external(x, intrablock[ib]));  // x += feature: d(feature) = d(x)
                        TRY(export_feature_grad(x, ib++));
                    }
                }
                skips.push_back(x);
            }
            if (lv.has_down) {
                Act y;
                TRY(R::conv3(x, nullptr, lv.down, 2, 0, nullptr, 0, 1, nullptr, ACT_NONE, &y));
                if (is_live(x)) {
                    live.insert(y.p);
                    const ConvW* cw = &lv.down;
                    const Act xin = x;
                    tape.push_back([=]() -> int {
                        auto it = slots.find(y.p);
                        MRISR_REQUIRE(it != slots.end() && it->second.written, "downsample output has no gradient");
                        Slot& sx = slot(xin);
                        Act dy = y; dy.p = it->second.g;
                        TRY(conv_dgrad(dy, *cw, 1, sx.g, sx.written));
                        sx.written = true;
                        return 0;
                    });
                }
                x = y;
                skips.push_back(x);
            }
            if (!has_attn && ib < n_intra) {
                // in place on the last skip (see Runner::encoder): d(feature) = d(x) with x's slot collecting the mid
                // block's AND the decoder's (skip) contributions
                TRY(R::add_external(x, intrablock[ib]));
                TRY(export_feature_grad(x, ib++));
            }
        }
        // ---- ControlNet residuals on the skips (after the whole down path, before the mid block: res_srdiff.py:73-78 /
        // diffusers `down_block_res_samples = [s + r for ...]`) ----
        if (!m.tr_down.empty()) {
            MRISR_REQUIRE(m.tr_down.size() == skips.size(), "one ControlNet residual per skip connection");
            for (size_t k = 0; k < skips.size(); ++k) {
                Act y;
                TRY(add_residual_t(skips[k], m.tr_down[k], k < m.d_tr_down.size() ? &m.d_tr_down[k] : nullptr, &y));
                skips[k] = y;
            }
        }
        // ---- mid ----
        {
            Act y;
            TRY(resnet_t(m.mid_r0, x, nullptr, &y));
            x = y;
            TRY(transformer_t(m.mid_xf, x, &y));
            x = y;
            TRY(resnet_t(m.mid_r1, x, nullptr, &y));
            x = y;
            if (m.has_tr_mid) {
                TRY(add_residual_t(x, m.tr_mid, m.d_tr_mid.data ? &m.d_tr_mid : nullptr, &y));
                x = y;
            }
        }
        // ---- decoder ----
        for (int i = 0; i < m.cfg.num_levels; ++i) {
            Level& lv = m.up[i];
            for (size_t j = 0; j < lv.res.size(); ++j) {
                Act sk = skips.back();
                skips.pop_back();
                Act y;
                TRY(resnet_t(lv.res[j], x, &sk, &y));
                x = y;
                if (!lv.xf.empty()) {
                    TRY(transformer_t(lv.xf[j], x, &y));
                    x = y;
                }
            }
            if (lv.has_up) {
                Act y;
                TRY(R::conv3(x, nullptr, lv.up, 1, 1, nullptr, 0, 1, nullptr, ACT_NONE, &y));
                if (is_live(x)) {
                    live.insert(y.p);
                    const ConvW* cw = &lv.up;
                    const Act xin = x;
                    tape.push_back([=]() -> int {
                        // y = conv(nearest_x2(x)):  dU = dgrad(dy) at the x2 size, dx = 2x2 sum pool of dU
                        auto it = slots.find(y.p);
                        MRISR_REQUIRE(it != slots.end() && it->second.written, "upsample output has no gradient");
                        Slot& sx = slot(xin);
                        const size_t mk = m.arena.mark();
                        Act dU = new_act(y.B, y.H, y.W, cw->cin);
                        if (!dU.p) return 7;
                        Act dy = y; dy.p = it->second.g;
                        TRY(conv_dgrad(dy, *cw, 0, dU.p, false));
                        if (!dry) TRY(launch_sumpool2<T>(dU.p, sx.g, xin.B, xin.H, xin.W, xin.C, sx.written ? 1 : 0, st));
                        sx.written = true;
                        m.arena.release(mk);
                        return 0;
                    });
                }
                x = y;
            }
        }
        // ---- head ----
        Act xn, y;
        float* gp = nullptr;
        int gns = 1;
        TRY(R::gn(x, nullptr, m.norm_out, true, m.cfg.norm_eps, &xn, &gp, &gns));
        if (m.conv_out.cout % 4 == 0) TRY(R::conv3(xn, nullptr, m.conv_out, 1, 0, nullptr, 0, 1, nullptr, ACT_NONE, &y));
        else TRY(R::direct(xn, m.conv_out, 1, ACT_NONE, nullptr, &y));
        if (pred_out) TRY(R::export_act(y, *pred_out, 1.0f));
        // ---- loss = mean((eps_hat - eps)^2), d(loss)/d(eps_hat) ----
        MRISR_REQUIRE(target.ndim == 4 && target.dtype == MRISR_F32 && target.layout == MRISR_NCHW && target.shape[0] == y.B &&
                          target.shape[1] == y.C && target.shape[2] == y.H && target.shape[3] == y.W,
                      "target: f32 NCHW of the prediction's shape");
        Act dy = new_act(y.B, y.H, y.W, y.C);
        if (!dy.p) return 7;
        if (!dry) {
            MRISR_CHECK_HIP(hipMemsetAsync(loss_dev, 0, sizeof(float), st));
            TRY(launch_mse_grad<T>(y.p, static_cast<const float*>(target.data), dy.p, loss_dev, y.B, y.C, y.H, y.W, st));
        }
        // ---- backward ----
        {
            MRISR_REQUIRE(is_live(x), "no trainable adapter reaches the output");
            Slot& sx = slot(x);
            const size_t mk = m.arena.mark();
            Act dxn = new_act(x.B, x.H, x.W, x.C);
            if (!dxn.p) return 7;
            TRY(conv_dgrad(dy, m.conv_out, 0, dxn.p, false));
            TRY(gn_bwd(x, nullptr, m.norm_out, true, m.cfg.norm_eps, gp, gns, dxn.p, sx.g, false, nullptr, false));
            sx.written = true;
            m.arena.release(mk);
        }
        for (size_t i = tape.size(); i-- > 0;) TRY(tape[i]());
        return 0;
    }
};

// ================================================================================================
// full-parameter training of a ControlNet handle
// ================================================================================================
template <typename T>
static int full_train_prepare_t(Model& m, hipStream_t st) {
    int err = 0;
    auto conv_dgrad = [&](ConvW& c) { pack_conv_dgrad<T>(m, c, st, err); };
    auto lin_t = [&](LinW& l) { pack_lin_t<T>(m, l, true, st, err); };
    for (auto& lv : m.down) {
        for (auto& r : lv.res) { conv_dgrad(r.c1); conv_dgrad(r.c2); if (r.has_sc) lin_t(r.sc); }
        if (lv.has_down) conv_dgrad(lv.down);
        for (auto& x : lv.xf) for (LinW* l : {&x.proj_in, &x.qkv, &x.out1, &x.q2, &x.out2, &x.ff1, &x.ff2, &x.proj_out}) lin_t(*l);
    }
    for (ResW* r : {&m.mid_r0, &m.mid_r1}) { conv_dgrad(r->c1); conv_dgrad(r->c2); if (r->has_sc) lin_t(r->sc); }
    for (LinW* l : {&m.mid_xf.proj_in, &m.mid_xf.qkv, &m.mid_xf.out1, &m.mid_xf.q2, &m.mid_xf.out2, &m.mid_xf.ff1, &m.mid_xf.ff2, &m.mid_xf.proj_out}) lin_t(*l);
    for (auto& l : m.cn_down) lin_t(l);
    lin_t(m.cn_mid);
    for (size_t k = 1; k < m.ce.size(); ++k) {  // condition embedding: zero-padded dgrad banks (layer 0 needs no input gradient)
        ConvW& c = m.ce[k];
        const RawParam* w = m.find(c.name + ".weight");
        if (!w || c.ks != 3) { err = 3; set_error("condition embedding: missing / unexpected layer " + c.name); break; }
        if (!c.wd) c.wd = m.new_packed((size_t)c.cout * c.cin * 9 * sizeof(T), false);
        if (!c.wd) { err = 4; break; }
        if (launch_pack_conv_dgrad_padded<T>(static_cast<const float*>(w->data->p), c.wd, (int)w->shape[0], (int)w->shape[1], c.cout, c.cin, st)) err = 5;
    }
    MRISR_CHECK_HIP(hipGetLastError());
    return err;
}

int Model::full_train_prepare(hipStream_t st) {
    MRISR_REQUIRE(finalized && is_controlnet, "full-parameter training is implemented for a finalized ControlNet handle");
    MRISR_REQUIRE(cfg.lora_rank == 0, "full-parameter training: no adapters on the ControlNet");
    full_off.clear();
    full_trainables.clear();
    full_unsupported.clear();
    long long off = 0;
    for (auto& kv : raw) {  // key order: the layout is a property of the parameter names alone
        const RawParam& r = kv.second;
        const long long rows = r.shape.empty() ? 1 : r.shape[0];
        full_off[kv.first] = off;
        full_trainables.push_back({kv.first, off, r.numel(), (int)rows, (int)(r.numel() / (rows ? rows : 1))});
        off += r.numel();
        // what this build differentiates: every conv / linear weight and bias of the encoder, mid block and zero convs, the affine
        // parameters of every norm, the time-embedding MLP and its per-block projections, the condition embedding - everything
        const std::string& k = kv.first;
        auto has = [&](const char* s) { return k.find(s) != std::string::npos; };
        (void)has;  // (every tensor is differentiated; full_unsupported stays empty)
    }
    n_full = off;
    return cfg.compute_dtype == MRISR_F32 ? full_train_prepare_t<float>(*this, st) : full_train_prepare_t<bf16>(*this, st);
}

int Model::full_train_bind(float* theta_dev, float* grad_dev, int init_from_model, hipStream_t st) {
    if (full_off.empty()) TRY(full_train_prepare(st));
    MRISR_REQUIRE(theta_dev && grad_dev, "theta / grad device buffers");
    full_theta = theta_dev;
    full_grad = grad_dev;
    if (init_from_model)
        for (auto& t : full_trainables)
            MRISR_CHECK_HIP(hipMemcpyAsync(theta_dev + t.offset, raw.at(t.key).data->p, (size_t)t.numel * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

// after an optimiser step: theta -> the f32 masters, every packed weight (forward and dgrad copies) rebuilt in place
int Model::full_train_refresh(hipStream_t st) {
    MRISR_REQUIRE(full_theta, "bind the trainable vector first");
    for (auto& t : full_trainables)
        MRISR_CHECK_HIP(hipMemcpyAsync(raw.at(t.key).data->p, full_theta + t.offset, (size_t)t.numel * sizeof(float), hipMemcpyDeviceToDevice, st));
    // re-pack INTO the existing buffers: the forward copies (finalize) and, still in the same buffer sequence, the dgrad copies
    repacking = true;
    repack_cursor = 0;
    int rc = finalize(st);
    if (!rc) rc = cfg.compute_dtype == MRISR_F32 ? full_train_prepare_t<float>(*this, st) : full_train_prepare_t<bf16>(*this, st);
    repacking = false;
    // finalize rebuilt the module structs: the per-block workspace pointers planned into them (cached context K / V^T, ...) are gone ->
    // plan again at the next forward (same sizes: no allocation, the dry passes only)
    ws_key.clear();
    train_ws_key.clear();
    cond_valid = false;
    ctx_valid = false;
    return rc;
}

template <typename T>
static int cn_forward_t(Model& m, const mrisr_tensor& sample, const long long* t, int t_scalar, const mrisr_tensor& ehs, const mrisr_tensor& cond,
                        float scale, mrisr_tensor* down_out, int n_down, mrisr_tensor* mid_out, hipStream_t st) {
    m.full_tape.reset();
    if (m.train_ws_key != m.ws_key) {  // dry pass of forward + backward sizes the arena exactly
        ++m.ws_gen;
        m.arena.dry = true;
        m.arena.reset();
        m.arena.peak = 0;
        int rc;
        {
            Trainer<T> tr(m, st, true);
            rc = tr.cn_forward(sample, t, t_scalar, ehs, cond, scale, down_out, n_down, mid_out);
            if (!rc) {
                std::vector<mrisr_tensor> dd(down_out, down_out + n_down);
                rc = tr.cn_backward(dd.data(), n_down, mid_out, scale);
            }
        }
        m.arena.dry = false;
        if (rc) return rc;
        MRISR_CHECK_HIP(hipStreamSynchronize(st));
        TRY(m.arena.buf.reserve(m.arena.peak + 4096, false));
        m.arena.reset();
        m.train_ws_key = m.ws_key;
    }
    auto tr = std::make_shared<Trainer<T>>(m, st, false);
    TRY(tr->cn_forward(sample, t, t_scalar, ehs, cond, scale, down_out, n_down, mid_out));
    m.full_tape = tr;
    return 0;
}

int Model::controlnet_train_forward(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs, const mrisr_tensor* cond,
                                    float scale, mrisr_tensor* down_out, int n_down, mrisr_tensor* mid_out, hipStream_t st) {
    MRISR_REQUIRE(is_controlnet && full_grad, "bind the ControlNet's trainable vector first (mrisr_controlnet_train_bind)");
    MRISR_REQUIRE(sample && sample->ndim == 4 && timestep && timestep->dtype == MRISR_I64 && ehs && ehs->ndim == 3 && cond && down_out && mid_out,
                  "ControlNet training forward: sample, timestep, encoder_hidden_states, controlnet_cond, outputs");
    const int B = (int)sample->shape[0], h = (int)sample->shape[2], w = (int)sample->shape[3];
    const int t_scalar = timestep->ndim == 0 || timestep->shape[0] == 1;
    MRISR_REQUIRE(t_scalar || timestep->shape[0] == B, "timestep length");
    keep = true;
    int rc = ensure_workspace(B, h, w, (int)ehs->shape[1], st);
    if (!rc) {
        const long long* t = static_cast<const long long*>(timestep->data);
        rc = cfg.compute_dtype == MRISR_F32 ? cn_forward_t<float>(*this, *sample, t, t_scalar, *ehs, *cond, scale, down_out, n_down, mid_out, st)
                                            : cn_forward_t<bf16>(*this, *sample, t, t_scalar, *ehs, *cond, scale, down_out, n_down, mid_out, st);
    }
    keep = false;
    return rc;
}

int Model::controlnet_train_backward(const mrisr_tensor* d_down, int n_down, const mrisr_tensor* d_mid, float scale, hipStream_t st) {
    MRISR_REQUIRE(full_tape, "run mrisr_controlnet_train_forward first (its recorded forward is consumed by ONE backward)");
    keep = true;
    int rc;
    if (cfg.compute_dtype == MRISR_F32) rc = static_cast<Trainer<float>*>(full_tape.get())->cn_backward(d_down, n_down, d_mid, scale);
    else rc = static_cast<Trainer<bf16>*>(full_tape.get())->cn_backward(d_down, n_down, d_mid, scale);
    keep = false;
    full_tape.reset();
    return rc;
}

// what a training step's workspace plan depends on besides the geometry (ws_key): the adapter features (their layout decides whether
// they pass through the arena) and which of them export a gradient (a frozen UNet differentiates its encoder only then).  Without
// features the key is ws_key itself, so a plan made with features is never reused without them, nor the reverse.
static std::string train_plan_key(const Model& m, const mrisr_tensor* intrablock, int n_intra) {
    if (n_intra <= 0 && m.d_intra.empty()) return m.ws_key;
    std::string k = m.ws_key + ",intra:";
    for (int i = 0; i < n_intra; ++i) k += intrablock[i].layout == MRISR_NHWC && intrablock[i].dtype == m.cfg.compute_dtype ? 'h' : 'c';
    k += ",d:";
    for (const mrisr_tensor& d : m.d_intra) k += d.data ? '1' : '0';
    return k;
}

template <typename T>
static int train_plan_t(Model& m, const mrisr_tensor& sample, const long long* t, int t_scalar, const mrisr_tensor& ehs,
                        const mrisr_tensor* intrablock, int n_intra, const mrisr_tensor& target, float* loss_dev,
                        const mrisr_tensor* pred_out, hipStream_t st) {
    const std::string key = train_plan_key(m, intrablock, n_intra);
    if (m.train_ws_key != key) {
        // dry pass of forward + backward sizes the arena exactly
        ++m.ws_gen;  // the arena may be reallocated below
        m.arena.dry = true;
        m.arena.reset();
        m.arena.peak = 0;
        int rc;
        {
            Trainer<T> tr(m, st, true);
            rc = tr.step(sample, t, t_scalar, ehs, intrablock, n_intra, target, loss_dev, pred_out);
        }
        m.arena.dry = false;
        if (rc) return rc;
        MRISR_CHECK_HIP(hipStreamSynchronize(st));
        TRY(m.arena.buf.reserve(m.arena.peak + 4096, false));
        m.arena.reset();
        m.train_ws_key = key;
    }
    return 0;
}

template <typename T>
static int train_step_t(Model& m, const mrisr_tensor& sample, const long long* t, int t_scalar, const mrisr_tensor& ehs,
                        const mrisr_tensor* intrablock, int n_intra, const mrisr_tensor& target, float* loss_dev,
                        const mrisr_tensor* pred_out, hipStream_t st) {
    TRY(train_plan_t<T>(m, sample, t, t_scalar, ehs, intrablock, n_intra, target, loss_dev, pred_out, st));
    Trainer<T> tr(m, st, false);
    return tr.step(sample, t, t_scalar, ehs, intrablock, n_intra, target, loss_dev, pred_out);
}

// the planning half of train_step alone (workspace + dry pass; both synchronise): what a stream capture of train_step needs done first
int Model::train_plan(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs, const mrisr_tensor* intrablock,
                      int n_intra, const mrisr_tensor* target, float* loss_dev, hipStream_t st) {
    MRISR_REQUIRE(train_ready && (n_trainable == 0 || (theta && grad)), "bind the trainable vector first (mrisr_train_bind)");
    MRISR_REQUIRE(sample && sample->ndim == 4 && timestep && ehs && ehs->ndim == 3 && target && loss_dev, "train_plan arguments");
    const int B = (int)sample->shape[0], h = (int)sample->shape[2], w = (int)sample->shape[3];
    const int t_scalar = timestep->ndim == 0 || timestep->shape[0] == 1;
    MRISR_REQUIRE(!pag.on(), "a training forward cannot be recorded while perturbed-attention guidance is set (mrisr_model_set_pag)");
    MRISR_REQUIRE(!freeu.on, "a training forward cannot be recorded while FreeU is on (mrisr_model_set_freeu)");
    MRISR_REQUIRE(!cond.on, "a training forward cannot be recorded while a sampler's conditioning table is set on the handle");
    keep = true;
    int rc = ensure_workspace(B, h, w, (int)ehs->shape[1], st);
    if (!rc) {
        const long long* t = static_cast<const long long*>(timestep->data);
        rc = cfg.compute_dtype == MRISR_F32 ? train_plan_t<float>(*this, *sample, t, t_scalar, *ehs, intrablock, n_intra, *target, loss_dev, nullptr, st)
                                            : train_plan_t<bf16>(*this, *sample, t, t_scalar, *ehs, intrablock, n_intra, *target, loss_dev, nullptr, st);
    }
    keep = false;
    return rc;
}

int Model::train_step(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs, const mrisr_tensor* intrablock,
                      int n_intra, const mrisr_tensor* target, float* loss_dev, mrisr_tensor* pred_out, hipStream_t st) {
    MRISR_REQUIRE(train_ready && (n_trainable == 0 || (theta && grad)), "bind the trainable vector first (mrisr_train_bind)");
    MRISR_REQUIRE(sample && sample->ndim == 4 && sample->shape[1] == cfg.in_channels, "sample must be [B, in_channels, h, w]");
    MRISR_REQUIRE(timestep && timestep->dtype == MRISR_I64 && timestep->ndim <= 1, "timestep: device int64, 0-dim or [B]");
    MRISR_REQUIRE(ehs && ehs->ndim == 3, "encoder_hidden_states must be [B, L, D]");
    MRISR_REQUIRE(target && loss_dev, "target / loss");
    const int B = (int)sample->shape[0], h = (int)sample->shape[2], w = (int)sample->shape[3];
    const int t_scalar = timestep->ndim == 0 || timestep->shape[0] == 1;
    MRISR_REQUIRE(t_scalar || timestep->shape[0] == B, "timestep length");
    MRISR_REQUIRE(!pag.on(), "a training forward cannot be recorded while perturbed-attention guidance is set (mrisr_model_set_pag)");
    MRISR_REQUIRE(!freeu.on, "a training forward cannot be recorded while FreeU is on (mrisr_model_set_freeu)");
    MRISR_REQUIRE(!cond.on, "a training forward cannot be recorded while a sampler's conditioning table is set on the handle");
    keep = true;
    int rc = ensure_workspace(B, h, w, (int)ehs->shape[1], st);
    if (!rc) {
        const long long* t = static_cast<const long long*>(timestep->data);
        rc = cfg.compute_dtype == MRISR_F32
                 ? train_step_t<float>(*this, *sample, t, t_scalar, *ehs, intrablock, n_intra, *target, loss_dev, pred_out, st)
                 : train_step_t<bf16>(*this, *sample, t, t_scalar, *ehs, intrablock, n_intra, *target, loss_dev, pred_out, st);
    }
    keep = false;
    return rc;
}

}  // namespace mrisr
