// T2I-Adapter: the model handle, its forward and backward as launch sequences over the handle's own arena (the backward through the
// two composites of train_ops.h, like the UNet / ControlNet trainer), its extern "C" entry points (mrisr_adapter_*) and the
// adapter_fit_* interface (model.h) that fit.hip drives inside its captured graphs.
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "api.h"
#include "model.h"
#include "train_ops.h"

using namespace mrisr;

// =================================================================================================
// T2I-Adapter (reference src/adapters/modules.py:114-157, sk=True)
// =================================================================================================
struct AdBlock {
    bool down = false, has_in = false;
    ConvW down_w, in_w, b1, b2;
    int in_c = 0, out_c = 0;
};
struct AdRec {  // what one block's backward needs (activations stay in the arena until the next forward)
    Act x_in, x_down, x_pre, hmid, y;
};
struct AdTrainable {
    std::string key;
    long long offset = 0, numel = 0;
    std::vector<int64_t> shape;
};
struct mrisr_adapter {
    mrisr_adapter_cfg cfg{};
    std::map<std::string, RawParam> raw;
    std::vector<std::unique_ptr<DevBuf>> packed;
    ConvW conv_in;
    std::vector<AdBlock> blocks;
    Arena arena;
    bool finalized = false;
    // ---- training (the adapter runs and is differentiated every step) ----
    bool train_ready = false, recorded = false;
    std::vector<AdTrainable> trainables;
    long long n_trainable = 0;
    float* theta = nullptr;
    float* grad = nullptr;
    Act rec_u;
    std::vector<AdRec> recs;
    Act bwd_dcur;             // running gradient between the level-wise backward calls
    int bwd_next_level = -1;  // next level mrisr_adapter_backward_level expects (descending)
    // the training loop's plan (adapter_fit_plan): geometry it was made for, bumped on every re-plan (captured graphs key on it);
    // an eager forward clears the key, since it resets (and may reallocate) the arena
    std::string fit_plan_key;
    unsigned long long fit_plan_gen = 0;
    std::vector<ConvW*> all_convs() {
        std::vector<ConvW*> v{&conv_in};
        for (auto& b : blocks) {
            if (b.down) v.push_back(&b.down_w);
            if (b.has_in) v.push_back(&b.in_w);
            v.push_back(&b.b1);
            v.push_back(&b.b2);
        }
        return v;
    }
};

template <typename T>
struct AdRunner {
    mrisr_adapter& a;
    hipStream_t st;
    bool dry;
    void* alloc(size_t bytes) {
        void* p = a.arena.alloc(bytes);
        if (!p) set_error("adapter workspace exhausted");
        return p;
    }
    Act new_act(int B, int H, int W, int C) {
        Act x; x.B = B; x.H = H; x.W = W; x.C = C;
        x.p = alloc(x.numel() * sizeof(T));
        return x;
    }
    // plans split-K (the partial sums live in the arena) and, unless dry, launches
    int gemm(GemmArgs& g) { return gemm_run<T>(g, st, dry, [this](size_t n) { return alloc(n); }); }
    int conv(const Act& x, const ConvW& cw, int stride, int act, const Act* resid, Act* out) {
        MRISR_REQUIRE(cw.cin == x.C, "adapter conv channel mismatch");
        const int Ho = (x.H - 1) / stride + 1, Wo = (x.W - 1) / stride + 1;
        *out = new_act(x.B, cw.ks == 3 ? Ho : x.H, cw.ks == 3 ? Wo : x.W, cw.cout);
        if (!out->p) return 7;
        GemmArgs g;
        ga_rows(g, x);
        if (cw.ks == 3) {
            ga_conv3(g, x, stride); ga_weight(g, cw.w, x.B * Ho * Wo, cw.cout, 9 * x.C);
        } else {
            MRISR_REQUIRE(stride == 1, "1x1 conv stride");
            ga_weight(g, cw.w, (int)x.rows(), cw.cout, x.C);
        }
        g.bias = cw.b; g.act = act; ga_resid(g, resid); ga_out(g, out->p, cw.cout);
        return gemm(g);
    }
    // ---- backward building blocks: the two composites of train_ops.h on this arena ----
    // dX = dgrad(dY) (+ resid);  3x3: conv with the flipped / transposed bank, stride 2 through zero-stuffing;  1x1: dY W
    int conv_dgrad(const Act& dy, const ConvW& cw, int stride, const Act* resid, Act* dx) {
        MRISR_REQUIRE(cw.wd && dy.C == cw.cout, "adapter dgrad weights");
        const int up = stride == 2 ? 1 : 0;
        *dx = new_act(dy.B, dy.H << up, dy.W << up, cw.cin);
        if (!dx->p) return 7;
        if (cw.ks == 3)
            return conv_dgrad_run<T>(st, dry, [this](GemmArgs& g) { return gemm(g); }, dy.p, dy.B, dy.H, dy.W, cw.cout, cw.cin, cw.wd, up,
                                     dx->p, resid ? resid->p : nullptr, resid ? resid->C : 0);
        GemmArgs g;
        ga_rows(g, dy.p, cw.cout, cw.cout); ga_weight(g, cw.wd, (int)dy.rows(), cw.cin, cw.cout); ga_resid(g, resid);
        ga_out(g, dx->p, cw.cin);
        return gemm(g);
    }
    // dW, db of y = conv(x), accumulated into the bound gradient vector
    int conv_wgrad(const Act& x, const Act& dy, const ConvW& cw, int stride) {
        MRISR_REQUIRE(cw.offW >= 0 && a.grad, "adapter gradient vector not bound");
        const size_t mk = a.arena.mark();
        TRY(conv_wgrad_run<T>(st, dry, [this](size_t n) { return alloc(n); }, [this](GemmArgs& g) { return gemm(g); }, x.p, x.B, x.H, x.W, x.C,
                              dy.p, dy.C, 0, dy.H, dy.W, cw.cout, cw.ks, stride, a.grad + cw.offW, cw.offB >= 0 ? a.grad + cw.offB : nullptr,
                              cw.cout, cw.cin, 0));
        a.arena.release(mk);
        return 0;
    }
    // d_feats: gradients w.r.t. the four feature maps (what mrisr_train_step wrote through mrisr_train_set_intrablock_grads)
    // Blocks k_hi .. k_lo (descending) of the backward; the running gradient lives in a.bwd_dcur between calls, so that the host
    // can cut the pass at level boundaries and start the exchange of a level's finished weight gradients while the lower
    // levels are still being differentiated (mrisr_adapter_backward_level).
    int backward_blocks(const mrisr_tensor* d_feats, int n_feats, int k_hi, int k_lo, bool with_conv_in) {
        MRISR_REQUIRE(a.recorded || dry, "run the adapter forward first");
        MRISR_REQUIRE(n_feats * a.cfg.nums_rb == (int)a.blocks.size(), "one feature gradient per level");
        Act dcur = a.bwd_dcur;
        for (int k = k_hi; k >= k_lo; --k) {
            AdBlock& b = a.blocks[k];
            AdRec& r = a.recs[k];
            if ((k + 1) % a.cfg.nums_rb == 0) {
                const mrisr_tensor& f = d_feats[(k + 1) / a.cfg.nums_rb - 1];
                MRISR_REQUIRE(f.ndim == 4 && f.shape[0] == r.y.B && f.shape[1] == r.y.C && f.shape[2] == r.y.H && f.shape[3] == r.y.W,
                              "adapter feature gradient shape");
                Act gf = new_act(r.y.B, r.y.H, r.y.W, r.y.C);
                if (!gf.p) return 7;
                if (!dry) {
                    if (f.layout == MRISR_NHWC) {
                        MRISR_REQUIRE(f.dtype == a.cfg.compute_dtype, "NHWC feature gradients use the compute dtype");
                        MRISR_CHECK_HIP(hipMemcpyAsync(gf.p, f.data, gf.numel() * sizeof(T), hipMemcpyDeviceToDevice, st));
                    } else {
                        TRY(launch_nchw_to_nhwc<T>(f.data, f.dtype, gf.p, gf.B, gf.C, gf.H, gf.W, st));
                    }
                    if (dcur.p) TRY(launch_add_inplace<T>(gf.p, dcur.p, (long long)gf.numel(), st));
                }
                dcur = gf;
            }
            MRISR_REQUIRE(dcur.p, "no gradient reaches the last adapter block");
            // y = block2(relu(block1(x_pre))) + x_pre
            TRY(conv_wgrad(r.hmid, dcur, b.b2, 1));
            Act dh, dx;
            TRY(conv_dgrad(dcur, b.b2, 1, nullptr, &dh));
            if (!dry) TRY(launch_relu_bwd<T>(dh.p, r.hmid.p, dh.p, (long long)dh.numel(), st));
            TRY(conv_wgrad(r.x_pre, dh, b.b1, 1));
            TRY(conv_dgrad(dh, b.b1, 1, &dcur, &dx));
            if (b.has_in) {
                TRY(conv_wgrad(r.x_down, dx, b.in_w, 1));
                Act d2;
                TRY(conv_dgrad(dx, b.in_w, 1, nullptr, &d2));
                dx = d2;
            }
            if (b.down) {
                TRY(conv_wgrad(r.x_in, dx, b.down_w, 2));
                Act d2;
                TRY(conv_dgrad(dx, b.down_w, 2, nullptr, &d2));
                dx = d2;
            }
            dcur = dx;
        }
        a.bwd_dcur = dcur;
        if (with_conv_in) return conv_wgrad(a.rec_u, dcur, a.conv_in, 1);
        return 0;
    }
    int backward(const mrisr_tensor* d_feats, int n_feats) {
        a.bwd_dcur = Act();
        a.bwd_next_level = -1;
        return backward_blocks(d_feats, n_feats, (int)a.blocks.size() - 1, 0, true);
    }
    // one level (nums_rb blocks) of the backward, levels in descending order; level 0 also differentiates conv_in
    int backward_level(const mrisr_tensor* d_feats, int n_feats, int level) {
        const int nlev = (int)a.blocks.size() / a.cfg.nums_rb;
        MRISR_REQUIRE(level >= 0 && level < nlev, "adapter level");
        if (level == nlev - 1) { a.bwd_dcur = Act(); a.bwd_next_level = level; }
        MRISR_REQUIRE(a.bwd_next_level == level, "adapter backward levels must run in descending order, starting at the top level");
        a.bwd_next_level = level - 1;
        return backward_blocks(d_feats, n_feats, (level + 1) * a.cfg.nums_rb - 1, level * a.cfg.nums_rb, level == 0);
    }

    int forward(const mrisr_tensor& x, mrisr_tensor* feats, int n_feats) {
        a.arena.reset();
        const int B = (int)x.shape[0], C = (int)x.shape[1], H = (int)x.shape[2], W = (int)x.shape[3];
        MRISR_REQUIRE(H % 8 == 0 && W % 8 == 0 && C * 64 == a.cfg.cin, "adapter input must be [B, cin/64, 8h, 8w]");
        Act u = new_act(B, H / 8, W / 8, C * 64);
        if (!u.p) return 7;
        if (!dry) TRY(launch_pixel_unshuffle_nchw<T>(x.data, x.dtype, u.p, B, C, H, W, 8, st));
        return forward_from(u, feats, n_feats);
    }
    // the forward from the already-unshuffled input u [B, H/8, W/8, cin] (compute dtype, NHWC); u must stay alive for the backward
    int forward_from(const Act& u, mrisr_tensor* feats, int n_feats) {
        Act cur;
        TRY(conv(u, a.conv_in, 1, ACT_NONE, nullptr, &cur));
        a.rec_u = u;
        a.recs.assign(a.blocks.size(), AdRec());
        int fi = 0;
        for (size_t k = 0; k < a.blocks.size(); ++k) {
            AdBlock& b = a.blocks[k];
            AdRec& rec = a.recs[k];
            Act y;
            rec.x_in = cur;
            if (b.down) { TRY(conv(cur, b.down_w, 2, ACT_NONE, nullptr, &y)); cur = y; }
            rec.x_down = cur;
            if (b.has_in) { TRY(conv(cur, b.in_w, 1, ACT_NONE, nullptr, &y)); cur = y; }
            rec.x_pre = cur;
            Act hmid;
            TRY(conv(cur, b.b1, 1, ACT_RELU, nullptr, &hmid));
            TRY(conv(hmid, b.b2, 1, ACT_NONE, &cur, &y));
            rec.hmid = hmid;
            rec.y = y;
            cur = y;
            if ((k + 1) % a.cfg.nums_rb == 0) {
                MRISR_REQUIRE(fi < n_feats, "too few feature outputs");
                const mrisr_tensor& f = feats[fi++];
                MRISR_REQUIRE(f.ndim == 4 && f.shape[0] == cur.B && f.shape[1] == cur.C && f.shape[2] == cur.H && f.shape[3] == cur.W,
                              "adapter feature output shape");
                if (!dry) {
                    if (f.layout == MRISR_NHWC) {
                        MRISR_REQUIRE(f.dtype == a.cfg.compute_dtype, "NHWC feature outputs use the compute dtype");
                        MRISR_CHECK_HIP(hipMemcpyAsync(f.data, cur.p, cur.numel() * sizeof(T), hipMemcpyDeviceToDevice, st));
                    } else {
                        TRY(launch_nhwc_to_nchw<T>(cur.p, f.data, f.dtype, cur.B, cur.C, cur.H, cur.W, 1.0f, st));
                    }
                }
            }
        }
        return 0;
    }
};

template <typename T>
static int adapter_finalize_t(mrisr_adapter& a, hipStream_t st) {
    a.packed.clear();
    a.blocks.clear();
    int err = 0;
    auto conv = [&](const std::string& name) {
        ConvW c;
        auto it = a.raw.find(name + ".weight");
        if (it == a.raw.end()) { set_error("missing parameter: " + name + ".weight"); err = 3; return c; }
        const RawParam& w = it->second;
        c.cout = (int)w.shape[0]; c.cin = (int)w.shape[1]; c.ks = (int)w.shape[2];
        c.name = name;
        a.packed.emplace_back(new DevBuf());
        if (a.packed.back()->reserve((size_t)w.numel() * sizeof(T), false)) { err = 4; return c; }
        c.w = a.packed.back()->p;
        if (launch_pack_conv3x3<T>(static_cast<const float*>(w.data->p), c.w, c.cout, c.cin, c.ks, st)) err = 5;
        auto ib = a.raw.find(name + ".bias");
        c.b = ib == a.raw.end() ? nullptr : static_cast<const float*>(ib->second.data->p);
        return c;
    };
    a.conv_in = conv("conv_in");
    int k = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < a.cfg.nums_rb; ++j, ++k) {
            AdBlock b;
            const std::string n = "body." + std::to_string(k);
            b.out_c = a.cfg.channels[i];
            b.in_c = (i > 0 && j == 0) ? a.cfg.channels[i - 1] : b.out_c;
            b.down = (i > 0 && j == 0);
            if (b.down) {
                if (!a.cfg.use_conv) { set_error("avg-pool downsample (use_conv=False) is not built"); return 8; }
                b.down_w = conv(n + ".down_opt.op");
            }
            if (a.raw.count(n + ".in_conv.weight")) { b.has_in = true; b.in_w = conv(n + ".in_conv"); }
            else if (b.in_c != b.out_c) { set_error("missing parameter: " + n + ".in_conv.weight"); return 3; }
            if (a.raw.count(n + ".skep.weight")) {
                // reference quirk: sk=False cannot run in the reference either
                set_error("Adapter_XL with sk=False is not runnable in the reference (channel mismatch in skep); use sk=True");
                return 8;
            }
            b.b1 = conv(n + ".block1");
            b.b2 = conv(n + ".block2");
            a.blocks.push_back(b);
        }
    if (err) return err;
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    a.finalized = true;
    return 0;
}

// re-pack every conv of the adapter (forward bank, dgrad bank, bias pointer) from the bound trainable vector
template <typename T>
static int adapter_repack_t(mrisr_adapter& a, hipStream_t st) {
    for (ConvW* c : a.all_convs()) {
        const float* w = a.theta + c->offW;
        TRY(launch_pack_conv3x3<T>(w, c->w, c->cout, c->cin, c->ks, st));
        if (c->ks == 3) TRY(launch_pack_conv_dgrad<T>(w, c->wd, c->cout, c->cin, st));
        else TRY(launch_transpose<T>(c->w, c->wd, c->cout, c->cin, c->cin, c->cout, 0, 0, 1, c->cout, st));
        if (c->offB >= 0) c->b = a.theta + c->offB;
    }
    return 0;
}
extern "C" {

int mrisr_adapter_create(const mrisr_adapter_cfg* cfg, mrisr_adapter** out) {
    API_BEGIN
    MRISR_REQUIRE(cfg && out, "null argument");
    MRISR_REQUIRE(cfg->compute_dtype == MRISR_F32 || cfg->compute_dtype == MRISR_BF16, "compute dtype");
    MRISR_REQUIRE(cfg->ksize == 1 || cfg->ksize == 3, "ksize 1 or 3");
    auto* a = new mrisr_adapter();
    a->cfg = *cfg;
    *out = a;
    return 0;
    API_END
}
void mrisr_adapter_destroy(mrisr_adapter* a) { delete a; }
int mrisr_adapter_set_param(mrisr_adapter* a, const char* key, const float* data, const int64_t* shape, int ndim,
                            int is_device) {
    API_BEGIN
    MRISR_REQUIRE(a && key && data, "null argument");
    RawParam rp;
    rp.shape.assign(shape, shape + ndim);
    rp.data = std::make_shared<DevBuf>();
    TRY(rp.data->reserve((size_t)rp.numel() * sizeof(float), false));
    MRISR_CHECK_HIP(hipMemcpy(rp.data->p, data, (size_t)rp.numel() * sizeof(float), is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    a->raw[key] = rp;
    a->finalized = false;
    return 0;
    API_END
}
int mrisr_adapter_finalize(mrisr_adapter* a, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(a, "null handle");
    TRY(gemm_prepare());
    if (a->cfg.compute_dtype == MRISR_F32) return adapter_finalize_t<float>(*a, (hipStream_t)stream);
    return adapter_finalize_t<bf16>(*a, (hipStream_t)stream);
    API_END
}
int mrisr_adapter_forward(mrisr_adapter* a, const mrisr_tensor* x, mrisr_tensor* feats, int n_feats, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(a && x && feats && a->finalized, "adapter not finalized / null argument");
    MRISR_REQUIRE(x->ndim == 4 && x->layout == MRISR_NCHW, "adapter input: NCHW image");
    hipStream_t st = (hipStream_t)stream;
    // size the arena with a dry pass (exact), then run
    int rc;
    a->fit_plan_key.clear();
    a->arena.dry = true; a->arena.reset(); a->arena.peak = 0;
    a->recorded = false;
    // training: the backward continues in the same arena (the activations must stay put), so size it for both now
    if (a->cfg.compute_dtype == MRISR_F32) { AdRunner<float> r{*a, st, true}; rc = r.forward(*x, feats, n_feats); if (!rc && a->train_ready) rc = r.backward(feats, n_feats); }
    else { AdRunner<bf16> r{*a, st, true}; rc = r.forward(*x, feats, n_feats); if (!rc && a->train_ready) rc = r.backward(feats, n_feats); }
    a->arena.dry = false;
    if (rc) return rc;
    if (a->arena.peak + 4096 > a->arena.buf.bytes) MRISR_CHECK_HIP(hipStreamSynchronize(st));  // the old buffer may still be in use
    TRY(a->arena.buf.reserve(a->arena.peak + 4096, false));
    if (a->cfg.compute_dtype == MRISR_F32) { AdRunner<float> r{*a, st, false}; rc = r.forward(*x, feats, n_feats); }
    else { AdRunner<bf16> r{*a, st, false}; rc = r.forward(*x, feats, n_feats); }
    a->recorded = rc == 0;
    return rc;
    API_END
}

// ---- T2I-Adapter training: flat f32 trainable / gradient vectors owned by the caller (as for the LoRA adapters) ----
int mrisr_adapter_train_prepare(mrisr_adapter* a, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(a && a->finalized, "adapter not finalized");
    if (a->train_ready) return 0;
    a->trainables.clear();
    long long off = 0;
    const size_t es = a->cfg.compute_dtype == MRISR_F32 ? 4 : 2;
    for (ConvW* c : a->all_convs()) {
        MRISR_REQUIRE(c->ks == 1 || c->ks == 3, "adapter conv kernel size");
        c->offW = off;
        a->trainables.push_back({c->name + ".weight", off, (long long)c->cout * c->cin * c->ks * c->ks, {c->cout, c->cin, c->ks, c->ks}});
        off += (long long)c->cout * c->cin * c->ks * c->ks;
        if (c->b) {
            c->offB = off;
            a->trainables.push_back({c->name + ".bias", off, c->cout, {c->cout}});
            off += c->cout;
        }
        a->packed.emplace_back(new DevBuf());
        TRY(a->packed.back()->reserve((size_t)c->cout * c->cin * c->ks * c->ks * es, false));
        c->wd = a->packed.back()->p;
    }
    a->n_trainable = off;
    a->train_ready = true;
    (void)stream;
    return 0;
    API_END
}
int64_t mrisr_adapter_train_num_trainable(const mrisr_adapter* a) { return a && a->train_ready ? (int64_t)a->n_trainable : -1; }
int mrisr_adapter_train_num_tensors(const mrisr_adapter* a) { return a && a->train_ready ? (int)a->trainables.size() : -1; }
int mrisr_adapter_train_tensor_info(const mrisr_adapter* a, int i, const char** key, int64_t* offset, int64_t shape[4], int* ndim) {
    MRISR_REQUIRE(a && a->train_ready && i >= 0 && i < (int)a->trainables.size() && key && offset && shape && ndim, "adapter trainable index");
    const AdTrainable& t = a->trainables[i];
    *key = t.key.c_str();
    *offset = t.offset;
    *ndim = (int)t.shape.size();
    for (size_t k = 0; k < t.shape.size(); ++k) shape[k] = t.shape[k];
    return 0;
}
int mrisr_adapter_train_refresh(mrisr_adapter* a, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(a && a->train_ready && a->theta, "bind the adapter's trainable vector first");
    return a->cfg.compute_dtype == MRISR_F32 ? adapter_repack_t<float>(*a, (hipStream_t)stream) : adapter_repack_t<bf16>(*a, (hipStream_t)stream);
    API_END
}
int mrisr_adapter_train_bind(mrisr_adapter* a, float* theta_dev, float* grad_dev, int init_from_model, void* stream) {
    API_BEGIN
    TRY(mrisr_adapter_train_prepare(a, stream));
    MRISR_REQUIRE(theta_dev && grad_dev, "theta / grad device buffers");
    a->theta = theta_dev;
    a->grad = grad_dev;
    if (init_from_model)
        for (auto& t : a->trainables) {
            auto it = a->raw.find(t.key);
            MRISR_REQUIRE(it != a->raw.end() && it->second.numel() == t.numel, "adapter tensor missing from the loaded parameters");
            MRISR_CHECK_HIP(hipMemcpyAsync(theta_dev + t.offset, it->second.data->p, (size_t)t.numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        }
    return mrisr_adapter_train_refresh(a, stream);
    API_END
}
int mrisr_adapter_backward(mrisr_adapter* a, const mrisr_tensor* d_feats, int n_feats, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(a && d_feats && a->train_ready && a->grad, "bind the adapter's trainable vector first");
    hipStream_t st = (hipStream_t)stream;
    if (a->cfg.compute_dtype == MRISR_F32) { AdRunner<float> r{*a, st, false}; return r.backward(d_feats, n_feats); }
    AdRunner<bf16> r{*a, st, false};
    return r.backward(d_feats, n_feats);
    API_END
}
int mrisr_adapter_backward_level(mrisr_adapter* a, const mrisr_tensor* d_feats, int n_feats, int level, void* stream) {
    API_BEGIN
    MRISR_REQUIRE(a && d_feats && a->train_ready && a->grad, "bind the adapter's trainable vector first");
    hipStream_t st = (hipStream_t)stream;
    if (a->cfg.compute_dtype == MRISR_F32) { AdRunner<float> r{*a, st, false}; return r.backward_level(d_feats, n_feats, level); }
    AdRunner<bf16> r{*a, st, false};
    return r.backward_level(d_feats, n_feats, level);
    API_END
}
int mrisr_adapter_train_level_range(const mrisr_adapter* ac, int level, int64_t* offset, int64_t* numel) {
    API_BEGIN
    mrisr_adapter* a = const_cast<mrisr_adapter*>(ac);
    MRISR_REQUIRE(a && a->train_ready && offset && numel, "adapter not prepared for training");
    const int rb = a->cfg.nums_rb, nlev = (int)a->blocks.size() / rb;
    MRISR_REQUIRE(level >= 0 && level < nlev, "adapter level");
    // all_convs() order = flat-vector order: conv_in, then per block (down, in_conv, block1, block2): a level is one contiguous range
    auto first_off = [&](AdBlock& b) { return b.down ? b.down_w.offW : (b.has_in ? b.in_w.offW : b.b1.offW); };
    const long long lo = level == 0 ? 0 : first_off(a->blocks[level * rb]);
    const long long hi = level + 1 < nlev ? first_off(a->blocks[(level + 1) * rb]) : a->n_trainable;
    *offset = lo;
    *numel = hi - lo;
    return 0;
    API_END
}

}  // extern "C"

// ---- the adapter inside mrisr.fit's captured graphs (fit.hip): planning split from the launches ----
namespace mrisr {

int adapter_fit_info(const mrisr_adapter* a, AdapterFitInfo* out) {
    MRISR_REQUIRE(a && out && a->finalized, "adapter not finalized");
    out->compute_dtype = a->cfg.compute_dtype;
    out->cin = a->cfg.cin;
    out->nums_rb = a->cfg.nums_rb;
    out->n_levels = a->cfg.nums_rb > 0 ? (int)a->blocks.size() / a->cfg.nums_rb : 0;
    for (int i = 0; i < 4; ++i) out->channels[i] = a->cfg.channels[i];
    out->n_trainable = a->train_ready ? a->n_trainable : 0;
    out->theta = a->theta;
    out->grad = a->grad;
    return 0;
}

static Act u_act(const mrisr_tensor& u) {
    Act x;
    x.p = u.data; x.B = (int)u.shape[0]; x.C = (int)u.shape[1]; x.H = (int)u.shape[2]; x.W = (int)u.shape[3];
    return x;
}

int adapter_fit_plan(mrisr_adapter* a, const mrisr_tensor* u, mrisr_tensor* feats, const mrisr_tensor* d_feats, int n_feats, hipStream_t st) {
    MRISR_REQUIRE(a && u && feats && d_feats && a->finalized && a->train_ready && a->theta && a->grad, "bind the adapter's trainable vector first");
    MRISR_REQUIRE(u->ndim == 4 && u->layout == MRISR_NHWC && u->dtype == a->cfg.compute_dtype && u->shape[1] == a->cfg.cin,
                  "adapter input activation: [B, cin, h, w] stored NHWC in the compute dtype");
    char kb[96];
    snprintf(kb, sizeof(kb), "B%lld,%lld,%lld,n%d", (long long)u->shape[0], (long long)u->shape[1], (long long)u->shape[2], n_feats);
    if (a->fit_plan_key == kb) return 0;
    const Act ua = u_act(*u);
    a->arena.dry = true; a->arena.reset(); a->arena.peak = 0;
    a->recorded = false;
    int rc;
    if (a->cfg.compute_dtype == MRISR_F32) {
        AdRunner<float> r{*a, st, true};
        rc = r.forward_from(ua, feats, n_feats);
        if (!rc) rc = r.backward(d_feats, n_feats);
    } else {
        AdRunner<bf16> r{*a, st, true};
        rc = r.forward_from(ua, feats, n_feats);
        if (!rc) rc = r.backward(d_feats, n_feats);
    }
    a->arena.dry = false;
    a->arena.reset();
    if (rc) return rc;
    MRISR_CHECK_HIP(hipStreamSynchronize(st));  // the old buffer may still be in use
    TRY(a->arena.buf.reserve(a->arena.peak + 4096, false));
    a->fit_plan_key = kb;
    ++a->fit_plan_gen;
    return 0;
}

int adapter_fit_forward(mrisr_adapter* a, const mrisr_tensor* u, mrisr_tensor* feats, int n_feats, hipStream_t st) {
    MRISR_REQUIRE(a && u && !a->fit_plan_key.empty(), "plan the adapter first (adapter_fit_plan)");
    a->arena.reset();
    int rc;
    if (a->cfg.compute_dtype == MRISR_F32) { AdRunner<float> r{*a, st, false}; rc = r.forward_from(u_act(*u), feats, n_feats); }
    else { AdRunner<bf16> r{*a, st, false}; rc = r.forward_from(u_act(*u), feats, n_feats); }
    a->recorded = rc == 0;
    return rc;
}

int adapter_fit_backward(mrisr_adapter* a, const mrisr_tensor* d_feats, int n_feats, hipStream_t st) {
    MRISR_REQUIRE(a && d_feats && a->train_ready && a->grad, "bind the adapter's trainable vector first");
    if (a->cfg.compute_dtype == MRISR_F32) { AdRunner<float> r{*a, st, false}; return r.backward(d_feats, n_feats); }
    AdRunner<bf16> r{*a, st, false};
    return r.backward(d_feats, n_feats);
}

int adapter_fit_repack(mrisr_adapter* a, hipStream_t st) {
    MRISR_REQUIRE(a && a->train_ready && a->theta, "bind the adapter's trainable vector first");
    return a->cfg.compute_dtype == MRISR_F32 ? adapter_repack_t<float>(*a, st) : adapter_repack_t<bf16>(*a, st);
}

std::string adapter_fit_key(const mrisr_adapter* ac) {
    mrisr_adapter* a = const_cast<mrisr_adapter*>(ac);
    char kb[128];
    snprintf(kb, sizeof(kb), ",ag%llu,aa%p,ath%p,agr%p", a->fit_plan_gen, a->arena.buf.p, (void*)a->theta, (void*)a->grad);
    std::string k = kb;
    for (ConvW* c : a->all_convs()) {
        snprintf(kb, sizeof(kb), ",%p/%p/%p", c->w, c->wd, (const void*)c->b);
        k += kb;
    }
    return k;
}

}  // namespace mrisr
