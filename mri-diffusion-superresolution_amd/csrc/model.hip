// Model runtime: weights keyed by diffusers state-dict names, load-time re-layout for the kernels, and the
// UNet2DConditionModel / ControlNetModel forward as a fixed sequence of kernel launches over a bump arena
// (deterministic addresses -> the whole step is hipGraph-capturable).  Spec: SURVEY.md App. A.1-A.6;
// reference call sites src/adapters/res_srdiff.py:65-78.
#include "model.h"
#include "runner.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace mrisr {

thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error_cstr() { return g_err.c_str(); }

// ================================================================================================
// parameters
// ================================================================================================
int Model::set_param(const char* key, const float* data, const int64_t* shape, int ndim, int is_device) {
    MRISR_REQUIRE(key && data && ndim >= 1 && ndim <= 4, "bad parameter");
    std::string k(key);
    // peft wraps a LoRA-targeted Linear: <mod>.base_layer.weight
    const std::string bl = ".base_layer.";
    size_t pos = k.find(bl);
    if (pos != std::string::npos) k = k.substr(0, pos) + "." + k.substr(pos + bl.size());
    RawParam rp;
    rp.shape.assign(shape, shape + ndim);
    const size_t bytes = (size_t)rp.numel() * sizeof(float);
    rp.data = std::make_shared<DevBuf>();
    TRY(rp.data->reserve(bytes, false));
    MRISR_CHECK_HIP(hipMemcpy(rp.data->p, data, bytes, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    raw[k] = rp;
    finalized = false;
    return 0;
}

int64_t Model::num_params() const {
    int64_t n = 0;
    for (auto& kv : raw) n += kv.second.numel();
    return n;
}

const RawParam* Model::find(const std::string& k) const {
    auto it = raw.find(k);
    return it == raw.end() ? nullptr : &it->second;
}

void* Model::new_packed(size_t bytes, bool zero) {
    if (repacking && repack_cursor < packed.size()) {  // re-pack after an optimiser step: the same sequence of buffers, no allocation
        DevBuf* b = packed[repack_cursor++].get();
        if (b->bytes < (bytes ? bytes : 16)) { set_error("re-pack: packed buffer sequence changed"); return nullptr; }
        if (zero && hipMemset(b->p, 0, bytes) != hipSuccess) return nullptr;
        return b->p;
    }
    packed.emplace_back(new DevBuf());
    if (packed.back()->reserve(bytes ? bytes : 16, zero)) return nullptr;
    return packed.back()->p;
}

template <typename T>
struct Packer {
    Model& m;
    hipStream_t st;
    int err = 0;
    explicit Packer(Model& mm, hipStream_t s) : m(mm), st(s) {}

    const RawParam* need(const std::string& k) {
        const RawParam* r = m.find(k);
        if (!r && !err) {  // keep the FIRST missing key as the message
            set_error("missing parameter: " + k);
            err = 3;
        }
        return r;
    }
    const float* f32(const std::string& k) {  // bias / gamma / beta stay f32: use the raw copy directly
        const RawParam* r = need(k);
        return r ? static_cast<const float*>(r->data->p) : nullptr;
    }
    NormW norm(const std::string& name) {
        NormW n;
        n.name = name;
        n.g = f32(name + ".weight");
        n.b = f32(name + ".bias");
        if (n.g) n.c = (int)m.find(name + ".weight")->shape[0];
        return n;
    }
    // lora_target (conv1 / conv2 of a UNet's ResnetBlock2D): a peft Conv2d adapter on the module is consumed - kept apart as the four views
    // of lora_conv.hip (lora_fused), or folded into the f32 weight before packing (merged mode), as linear() does
    ConvW conv(const std::string& name, bool lora_target = false) {
        ConvW c;
        const RawParam* w = need(name + ".weight");
        if (!w) return c;
        c.name = name;
        c.cout = (int)w->shape[0];
        c.cin = (int)w->shape[1];
        c.ks = (int)w->shape[2];
        c.w = m.new_packed((size_t)w->numel() * sizeof(T), false);
        if (!c.w) { err = 4; return c; }
        const float* wsrc = static_cast<const float*>(w->data->p);
        const RawParam* la = lora_target && !m.is_controlnet ? m.find(name + ".lora_A.default.weight") : nullptr;
        const RawParam* lb = la ? m.find(name + ".lora_B.default.weight") : nullptr;
        const bool fused_lora = m.cfg.lora_rank > 0 && m.cfg.lora_fused;
        const int r = la ? (int)la->shape[0] : 0;
        if (la && m.dora) { set_error("DoRA covers the linear targets only: conv adapter on " + name); err = 6; return c; }
        if (la && lb) {
            if (c.ks != 3 || la->numel() != (int64_t)r * c.cin * 9 || lb->numel() != (int64_t)c.cout * r || (int)lb->shape[0] != c.cout) {
                set_error("conv LoRA: lora_A [r, cin, 3, 3] / lora_B [cout, r, 1, 1] expected on " + name);
                err = 6;
                return c;
            }
        }
        std::unique_ptr<DevBuf> merged;
        if (la && lb && !fused_lora) {  // W' = W + s B A on [cout][cin * 9] (A's rows in the same [cin][3][3] order)
            merged.reset(new DevBuf());
            if (merged->reserve((size_t)w->numel() * sizeof(float), false)) { err = 4; return c; }
            if (merge_lora(wsrc, static_cast<const float*>(la->data->p), static_cast<const float*>(lb->data->p), static_cast<float*>(merged->p), c.cout,
                           c.cin * 9, r))
                err = 6;
            wsrc = static_cast<const float*>(merged->p);
        }
        if (launch_pack_conv3x3<T>(wsrc, c.w, c.cout, c.cin, c.ks, st)) err = 5;
        if (merged) (void)hipStreamSynchronize(st);  // merged buffer dies at scope end
        c.b = m.find(name + ".bias") ? f32(name + ".bias") : nullptr;
        if (la && lb && fused_lora) {
            if (r % 4 != 0 || r > 16) { set_error("conv LoRA: rank 4 / 8 / 12 / 16: " + name); err = 6; return c; }
            c.r = r;
            c.loraA = m.new_packed((size_t)r * 9 * c.cin * sizeof(T), false);
            if (sizeof(T) == 2) c.loraAd = m.new_packed((size_t)c.cin * conv_lora_kpad(r) * 2, true);
            c.loraB = static_cast<float*>(m.new_packed((size_t)c.cout * r * sizeof(float), false));
            c.loraBT = m.new_packed((size_t)r * c.cout * sizeof(T), false);
            if (!c.loraA || (sizeof(T) == 2 && !c.loraAd) || !c.loraB || !c.loraBT) { err = 4; return c; }
            if (launch_conv_lora_pack<T>(static_cast<const float*>(la->data->p), static_cast<const float*>(lb->data->p), m.lora_scale, c.loraA, c.loraAd,
                                         c.loraB, c.loraBT, c.cin, c.cout, r, st))
                err = 5;
        }
        return c;
    }
    // 3x3 conv with its channel counts padded up to multiples of `quantum` (zero filter rows / columns, zero bias): a narrow
    // layer (the ControlNet condition embedding: 16 / 32 / 96 channels) then runs through the implicit-GEMM kernels, and its
    // padded outputs are exact zeros (SiLU(0) = 0) that the next padded layer multiplies by zero columns.
    ConvW conv_padded(const std::string& name, bool pad_in, bool pad_out, int quantum) {
        ConvW c;
        const RawParam* w = need(name + ".weight");
        if (!w) return c;
        c.name = name;
        const int cout = (int)w->shape[0], cin = (int)w->shape[1];
        c.ks = (int)w->shape[2];
        c.cout = pad_out ? (cout + quantum - 1) / quantum * quantum : cout;
        c.cin = pad_in ? (cin + quantum - 1) / quantum * quantum : cin;
        c.w = m.new_packed((size_t)c.cout * c.cin * c.ks * c.ks * sizeof(T), false);
        if (!c.w) { err = 4; return c; }
        if (launch_pack_conv3x3_padded<T>(static_cast<const float*>(w->data->p), c.w, cout, cin, c.ks, c.cout, c.cin, st)) err = 5;
        if (const RawParam* b = m.find(name + ".bias")) {
            float* pb = static_cast<float*>(m.new_packed((size_t)c.cout * sizeof(float), true));
            if (!pb) { err = 4; return c; }
            if (hipMemcpyAsync(pb, b->data->p, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) err = 5;
            c.b = pb;
        }
        return c;
    }
    // Linear / 1x1 conv, optionally several modules fused along N (QKV, KV), optional LoRA, optional GEGLU.
    LinW linear(const std::vector<std::string>& mods, bool geglu = false) {
        LinW l;
        const bool fused_lora = m.cfg.lora_rank > 0 && m.cfg.lora_fused;
        int ntot = 0, k = 0;
        bool any_lora = false;
        int rmod = 0, nmod0 = 0;
        for (auto& mod : mods) {
            const RawParam* w = need(mod + ".weight");
            if (!w) return l;
            ntot += (int)w->shape[0];
            k = (int)w->shape[1];
            const RawParam* la = m.find(mod + ".lora_A.default.weight");
            if (la) { any_lora = true; rmod = (int)la->shape[0]; }
            if (!nmod0) nmod0 = (int)w->shape[0];
        }
        l.n = ntot;
        l.k = k;
        l.geglu_half = geglu ? ntot / 2 : 0;
        l.mod_names = mods;
        for (auto& mod : mods) l.mod_lora.push_back(m.find(mod + ".lora_A.default.weight") ? 1 : 0);
        float* lbuf = nullptr;
        int ktot = k;
        if (any_lora && fused_lora) {
            // one rank-r adapter slot per fused module (modules without an adapter keep zero A rows / B rows)
            if (!lora_rank_low(rmod) && !lora_rank_high(rmod)) { set_error("LoRA rank 4 / 8 / 12 / 16 or 32 .. 128 in steps of 16: " + mods[0]); err = 6; return l; }
            l.r = rmod;
            l.secN = nmod0;
            if (lora_rank_high(rmod)) {  // the adapters as extra K columns of the projection
                if (m.cfg.fp8_linears || m.cfg.fp8_attention || m.cfg.fp8_train) { set_error("LoRA rank above 16 with fp8: the fp8 LoRA rows are a 16-row buffer"); err = 6; return l; }
                l.rp = lora_hr_rp(rmod, (int)sizeof(T));
                l.R = lora_hr_Rp(rmod, (int)mods.size(), (int)sizeof(T));
                ktot = k + l.R;
                l.loraA = m.new_packed((size_t)l.R * k * sizeof(T), true);
                if (!l.loraA) { err = 4; return l; }
            } else {
                l.R = (int)mods.size() * rmod;
                l.loraA = m.new_packed((size_t)l.R * k * sizeof(T), true);
                lbuf = static_cast<float*>(m.new_packed((size_t)ntot * rmod * sizeof(float), true));
                if (!l.loraA || !lbuf) { err = 4; return l; }
                l.loraB = lbuf;
                l.loraB_rw = lbuf;
            }
        }
        l.w = m.new_packed((size_t)ntot * ktot * sizeof(T), l.rp != 0);
        if (!l.w) { err = 4; return l; }
        bool has_bias = false;
        for (auto& mod : mods) has_bias |= m.find(mod + ".bias") != nullptr;
        float* bias = nullptr;
        if (has_bias) {
            bias = static_cast<float*>(m.new_packed((size_t)ntot * sizeof(float), true));
            if (!bias) { err = 4; return l; }
        }
        if (m.dora && any_lora && fused_lora) {  // g = m / ||W + s B A|| per packed row (rows of modules without an adapter: unused)
            l.dora_g = static_cast<float*>(m.new_packed((size_t)ntot * sizeof(float), true));
            if (!l.dora_g) { err = 4; return l; }
        }
        int row = 0, rcol = 0;
        for (auto& mod : mods) {
            const RawParam* w = m.find(mod + ".weight");
            const int n = (int)w->shape[0];
            const float* wsrc = static_cast<const float*>(w->data->p);
            const RawParam* la = m.find(mod + ".lora_A.default.weight");
            const RawParam* lb = m.find(mod + ".lora_B.default.weight");
            const RawParam* mg = dora_magnitude(mod, la && lb, n);
            if (err) return l;
            std::unique_ptr<DevBuf> merged;
            if (la && lb && !fused_lora) {
                // merged mode: W' = W + s * B A (DoRA: g (W + s B A)), computed in f32 on the device
                wsrc = merge_adapter(wsrc, la, lb, mg, merged, n, k);
                if (!wsrc) return l;
            }
            if (mg && fused_lora) {  // DoRA, adapter apart: the rows of this module are g W
                if (launch_dora_scale<T>(wsrc, static_cast<const float*>(la->data->p), static_cast<const float*>(lb->data->p),
                                         static_cast<const float*>(mg->data->p), m.lora_scale, l.dora_g, l.w, ktot, row, n, k, (int)la->shape[0],
                                         geglu ? n / 2 : 0, 0, st))
                    err = 5;
            } else if (launch_pack_rows<T>(wsrc, n, k, l.w, ktot, row, 0, geglu ? 1 : 0, n / 2, 1.0f, st)) err = 5;
            if (la && lb && fused_lora) {
                const int r = (int)la->shape[0];
                if (r != l.r || n != l.secN) { set_error("fused LoRA needs the same rank / width for every fused module: " + mod); err = 6; }
                // A rows -> loraA[rcol .. rcol+r);  (alpha/r) * B -> f32 [n][r] rows of this module (GEGLU: interleaved like the weight rows)
                if (err) return l;
                if (launch_pack_rows<T>(static_cast<const float*>(la->data->p), r, k, l.loraA, k, rcol, 0, 0, 0, 1.0f, st)) err = 5;
                if (mg) {  // DoRA: g (alpha/r) B, into the same places
                    if (l.rp ? launch_dora_pack_b<T>(static_cast<const float*>(lb->data->p), l.dora_g, m.lora_scale, l.w, ktot, row,
                                                     lora_hr_wcol(k, rcol / l.rp, l.rp), n, r, geglu ? n / 2 : 0, st)
                             : launch_dora_pack_b<float>(static_cast<const float*>(lb->data->p), l.dora_g, m.lora_scale, lbuf, r, row, 0, n, r,
                                                         geglu ? n / 2 : 0, st))
                        err = 5;
                } else if (l.rp) {  // (alpha/r) * B -> columns k + rcol .. of this module's rows of w
                    if (launch_pack_rows<T>(static_cast<const float*>(lb->data->p), n, r, l.w, ktot, row, lora_hr_wcol(k, rcol / l.rp, l.rp), geglu ? 1 : 0, n / 2, m.lora_scale, st)) err = 5;
                } else if (launch_pack_rows<float>(static_cast<const float*>(lb->data->p), n, r, lbuf, r, row, 0, geglu ? 1 : 0, n / 2, m.lora_scale, st)) err = 5;
            }
            if (fused_lora && any_lora) rcol += l.rp ? l.rp : l.r;
            if (const RawParam* b = m.find(mod + ".bias")) {
                const float* bsrc = static_cast<const float*>(b->data->p);
                if (geglu) {
                    if (launch_pack_bias_geglu(bsrc, bias + row, n / 2, st)) err = 5;
                } else if (hipMemcpyAsync(bias + row, bsrc, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) err = 5;
            }
            if (merged) (void)hipStreamSynchronize(st);  // merged buffer dies at scope end
            row += n;
        }
        l.b = bias;
        // fp8 copies (BASELINE configs[4]): the short-K projections the row-panel kernel serves
        // (fp8_linears 1: K = 320 only - at K = 640 the fp8 kernel's resident rows + their fp8 copy spill and it loses to the bf16
        // kernels, profiles/r02e_shape_fp8.log; 2: both widths)
        if (m.cfg.fp8_linears && sizeof(T) == 2 && (k == 320 || (k == 640 && m.cfg.fp8_linears >= 2)) && ntot % 16 == 0) {
            l.w8 = m.new_packed((size_t)ntot * k, false);
            l.w_scale = static_cast<float*>(m.new_packed((size_t)ntot * sizeof(float), true));
            if (!l.w8 || !l.w_scale) { err = 4; return l; }
            if (launch_quant_rows_fp8(l.w, ntot, k, l.w8, l.w_scale, st)) err = 5;
            if (l.R && l.R <= 16) {
                l.loraA8 = m.new_packed((size_t)16 * k, true);
                l.loraA_scale = static_cast<float*>(m.new_packed(16 * sizeof(float), true));
                if (!l.loraA8 || !l.loraA_scale) { err = 4; return l; }
                if (launch_quant_rows_fp8(l.loraA, l.R, k, l.loraA8, l.loraA_scale, st)) err = 5;
            }
        }
        return l;
    }
    // host-side helper for merged mode (load time only): W' = W + s*B*A via a tiny kernel
    int merge_lora(const float* w, const float* A, const float* B, float* out, int n, int k, int r);
    // the magnitude of a DoRA module (null: not a DoRA module).  A DoRA handle wants one [n] vector on every adapted linear; any other
    // handle wants none
    const RawParam* dora_magnitude(const std::string& mod, bool adapted, int n) {
        const RawParam* mg = m.find(mod + ".lora_magnitude_vector.default.weight");
        if (mg && !m.dora) { set_error("DoRA magnitude on a handle that is not a DoRA handle (use_dora=True): " + mod); err = 6; return nullptr; }
        if (!m.dora) return nullptr;
        if (mg && !adapted) { set_error("DoRA magnitude without lora_A / lora_B: " + mod); err = 6; return nullptr; }
        if (adapted && !mg) { set_error("DoRA adapter without its lora_magnitude_vector: " + mod); err = 6; return nullptr; }
        if (mg && (mg->shape.size() != 1 || mg->numel() != n)) { set_error("DoRA magnitude must be [out_features]: " + mod); err = 6; return nullptr; }
        return mg;
    }
    // merged mode: W + s B A - or, DoRA, g (W + s B A) with g = m / ||W + s B A|| per row - in f32 in `hold` (null: error)
    const float* merge_adapter(const float* w, const RawParam* la, const RawParam* lb, const RawParam* mg, std::unique_ptr<DevBuf>& hold, int n, int k) {
        hold.reset(new DevBuf());
        if (hold->reserve(((size_t)n * k + (mg ? n : 0)) * sizeof(float), false)) { err = 4; return nullptr; }  // DoRA: g behind the rows
        float* out = static_cast<float*>(hold->p);
        const float *A = static_cast<const float*>(la->data->p), *B = static_cast<const float*>(lb->data->p);
        const int r = (int)la->shape[0];
        if (mg ? launch_dora_scale<float>(w, A, B, static_cast<const float*>(mg->data->p), m.lora_scale, out + (size_t)n * k, out, k, 0, n, k, r, 0, 1, st)
               : merge_lora(w, A, B, out, n, k, r)) { err = 6; return nullptr; }
        return out;
    }
    // the f32 weight [n][k] a module multiplies by, as linear() packs it: the master copy, or - an adapter in merged mode (lora_fused = 0) -
    // W + s B A in `hold`
    const float* effective_f32(const std::string& mod, int n, int k, std::unique_ptr<DevBuf>& hold) {
        const RawParam* w = need(mod + ".weight");
        if (!w) return nullptr;
        const RawParam* la = m.find(mod + ".lora_A.default.weight");
        const RawParam* lb = m.find(mod + ".lora_B.default.weight");
        if (!(la && lb) || (m.cfg.lora_rank > 0 && m.cfg.lora_fused)) return static_cast<const float*>(w->data->p);
        const RawParam* mg = dora_magnitude(mod, true, n);
        if (err) return nullptr;
        return merge_adapter(static_cast<const float*>(w->data->p), la, lb, mg, hold, n, k);
    }

    ResW resnet(const std::string& name) {
        ResW r;
        r.n1 = norm(name + ".norm1");
        r.c1 = conv(name + ".conv1", true);
        r.n2 = norm(name + ".norm2");
        r.c2 = conv(name + ".conv2", true);
        r.cin = r.c1.cin;
        r.cout = r.c1.cout;
        if (m.find(name + ".conv_shortcut.weight")) {
            r.has_sc = true;
            r.sc = linear({name + ".conv_shortcut"});
            // the fused bank (built from the packed bf16 weights: the same rounded values both forms multiply); channel counts that fill K tiles
            // (a resnet with an un-merged conv adapter runs the literal sequence: no fused bank)
            if (sizeof(T) == 2 && !err && !r.c1.r && !r.c2.r && r.c2.w && r.sc.w && !r.sc.R && !r.sc.w8 && r.c2.b && r.sc.b && r.c2.ks == 3 && r.c2.cin == r.cout &&
                r.sc.k == r.cin && r.sc.n == r.cout && r.cin % 64 == 0 && r.cout % 64 == 0) {
                const size_t k2 = (size_t)9 * r.cout, kt = k2 + r.cin;
                r.c2sc = m.new_packed((size_t)r.cout * kt * sizeof(T), false);
                float* bs = static_cast<float*>(m.new_packed((size_t)r.cout * sizeof(float), false));
                if (!r.c2sc || !bs) { err = 4; return r; }
                if (hipMemcpy2DAsync(r.c2sc, kt * sizeof(T), r.c2.w, k2 * sizeof(T), k2 * sizeof(T), r.cout, hipMemcpyDeviceToDevice, st) != hipSuccess ||
                    hipMemcpy2DAsync(static_cast<T*>(r.c2sc) + k2, kt * sizeof(T), r.sc.w, (size_t)r.cin * sizeof(T), (size_t)r.cin * sizeof(T), r.cout,
                                     hipMemcpyDeviceToDevice, st) != hipSuccess ||
                    hipMemcpyAsync(bs, r.c2.b, (size_t)r.cout * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
                    launch_add_inplace<float>(bs, r.sc.b, r.cout, st))
                    err = 5;
                r.b2sc = bs;
            }
        }
        m.temb_mods.push_back(name + ".time_emb_proj");
        r.temb_off = m.tproj_total;
        m.tproj_total += r.cout;
        return r;
    }
    XfW transformer(const std::string& name) {
        XfW x;
        x.norm = norm(name + ".norm");
        x.C = x.norm.c;
        x.proj_in = linear({name + ".proj_in"});
        x.proj_out = linear({name + ".proj_out"});
        const std::string b = name + ".transformer_blocks.0";
        x.ln1 = norm(b + ".norm1");
        x.ln2 = norm(b + ".norm2");
        x.ln3 = norm(b + ".norm3");
        x.qkv = linear({b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"});
        x.out1 = linear({b + ".attn1.to_out.0"});
        x.q2 = linear({b + ".attn2.to_q"});
        x.kv2 = linear({b + ".attn2.to_k", b + ".attn2.to_v"});
        x.out2 = linear({b + ".attn2.to_out.0"});
        x.ff1 = linear({b + ".ff.net.0.proj"}, true);
        x.ff2 = linear({b + ".ff.net.2"});
        // fused feed-forward (gemm.hip mlp_fused_kernel): FF2's weight once more, K permuted to FF1's accumulator order
        if (sizeof(T) == 2 && !err && mlp_fused_ok(x.C, x.ff2.k, x.ff2.n) && x.ff1.n == 2 * x.ff2.k && !x.ff1.R && !x.ff2.R) {
            x.ff2p = m.new_packed((size_t)x.ff2.n * x.ff2.k * sizeof(T), false);
            if (!x.ff2p) { err = 4; return x; }
            if (launch_pack_mlp_w2(x.ff2.w, x.ff2p, x.ff2.n, x.ff2.k, st)) err = 5;
            if (!err && !x.proj_out.R && x.proj_out.n == 320 && x.proj_out.k == 320 && !x.proj_out.w8) {
                x.proj_outp = m.new_packed((size_t)320 * 320 * sizeof(T), false);
                if (!x.proj_outp) { err = 4; return x; }
                if (launch_pack_mlp_w2(x.proj_out.w, x.proj_outp, 320, 320, st)) err = 5;
            }
        }
        // ff.net.2 composed with proj_out (the blocks the fused feed-forward kernel does not take): [Wp W2 | Wp] and Wp b2 + bp, the product from
        // the f32 masters (a merged adapter included), the tail columns the packed proj_out.w itself
        if (sizeof(T) == 2 && !err && !mlp_fused_ok(x.C, x.ff2.k, x.ff2.n) && x.C % 64 == 0 && x.ff2.k == 4 * x.C && x.ff2.n == x.C &&
            x.proj_out.n == x.C && x.proj_out.k == x.C && !x.ff2.R && !x.proj_out.R && !x.ff2.w8 && !x.proj_out.w8 && x.ff2.w && x.proj_out.w) {
            const int C = x.C, K4 = 4 * C, Kt = 5 * C;
            x.ffpo = m.new_packed((size_t)C * Kt * sizeof(T), false);
            float* bs = static_cast<float*>(m.new_packed((size_t)C * sizeof(float), false));
            if (!x.ffpo || !bs) { err = 4; return x; }
            std::unique_ptr<DevBuf> hp, h2;
            const float* wp = effective_f32(name + ".proj_out", C, C, hp);
            const float* w2 = effective_f32(b + ".ff.net.2", C, K4, h2);
            const RawParam* b2 = m.find(b + ".ff.net.2.bias");
            const RawParam* bp = m.find(name + ".proj_out.bias");
            if (!wp || !w2) return x;
            if (launch_compose_ff_proj(wp, w2, b2 ? static_cast<const float*>(b2->data->p) : nullptr, bp ? static_cast<const float*>(bp->data->p) : nullptr,
                                       x.ffpo, Kt, bs, C, K4, st) ||
                hipMemcpy2DAsync(static_cast<T*>(x.ffpo) + K4, (size_t)Kt * sizeof(T), x.proj_out.w, (size_t)C * sizeof(T), (size_t)C * sizeof(T), C,
                                 hipMemcpyDeviceToDevice, st) != hipSuccess)
                err = 5;
            x.bffpo = bs;
            if (hp || h2) (void)hipStreamSynchronize(st);  // merged buffers die at scope end
        }
        // fused middle (xtail.hip xattn_tail_kernel): to_q / to_out of attn2 read their row operand in accumulator order
        if (sizeof(T) == 2 && !err && x.C == 320 && m.cfg.num_heads == 8 && x.q2.n == 320 && x.q2.k == 320 && x.out2.n == 320 && x.out2.k == 320 &&
            x.out1.n == 320 && x.out1.k == 320 && !m.cfg.fp8_linears && !x.q2.rp && !x.out2.rp && !x.out1.rp) {
            x.q2p = m.new_packed((size_t)320 * 320 * sizeof(T), false);
            x.out2p = m.new_packed((size_t)320 * 320 * sizeof(T), false);
            if (!x.q2p || !x.out2p) { err = 4; return x; }
            if (launch_pack_mlp_w2(x.q2.w, x.q2p, 320, 320, st) || launch_pack_mlp_w2(x.out2.w, x.out2p, 320, 320, st)) err = 5;
        }
        return x;
    }
};

__global__ void merge_lora_kernel(const float* w, const float* A, const float* B, float* out, int n, int k, int r,
                                  float s) {
    const long long total = (long long)n * k;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / k), col = (int)(i - (long long)row * k);
        float acc = 0.f;
        for (int j = 0; j < r; ++j) acc += B[(size_t)row * r + j] * A[(size_t)j * k + col];
        out[i] = w[i] + s * acc;
    }
}
template <typename T>
int Packer<T>::merge_lora(const float* w, const float* A, const float* B, float* out, int n, int k, int r) {
    long long blocks = ((long long)n * k + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(merge_lora_kernel, dim3((unsigned)blocks), dim3(256), 0, st, w, A, B, out, n, k, r, m.lora_scale);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}

template <typename T>
static int finalize_t(Model& m, hipStream_t st) {
    Packer<T> pk(m, st);
    const mrisr_unet_cfg& c = m.cfg;
    if (m.dora) {
        MRISR_REQUIRE(!m.is_controlnet, "DoRA on a ControlNet handle is not supported");
        MRISR_REQUIRE(!c.fp8_linears && !c.fp8_attention && !c.fp8_train, "DoRA cannot be combined with the fp8 modes");
    }
    if (!m.repacking) m.packed.clear();
    m.temb_mods.clear();
    m.tproj_total = 0;
    m.down.clear();
    m.up.clear();
    m.conv_in = pk.conv("conv_in");
    m.te1 = pk.linear({"time_embedding.linear_1"});
    m.te2 = pk.linear({"time_embedding.linear_2"});
    const int L = c.num_levels;
    for (int i = 0; i < L; ++i) {
        Level lv;
        for (int j = 0; j < c.layers_per_block; ++j) lv.res.push_back(pk.resnet("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j)));
        if (c.attn_levels[i])
            for (int j = 0; j < c.layers_per_block; ++j) lv.xf.push_back(pk.transformer("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j)));
        if (i < L - 1) {
            lv.has_down = true;
            lv.down = pk.conv("down_blocks." + std::to_string(i) + ".downsamplers.0.conv");
        }
        m.down.push_back(std::move(lv));
    }
    m.mid_r0 = pk.resnet("mid_block.resnets.0");
    m.mid_xf = pk.transformer("mid_block.attentions.0");
    m.mid_r1 = pk.resnet("mid_block.resnets.1");
    if (!m.is_controlnet) {
        for (int i = 0; i < L; ++i) {
            const int lvl = L - 1 - i;
            Level lv;
            for (int j = 0; j < c.layers_per_block + 1; ++j) lv.res.push_back(pk.resnet("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j)));
            if (c.attn_levels[lvl])
                for (int j = 0; j < c.layers_per_block + 1; ++j) lv.xf.push_back(pk.transformer("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j)));
            if (i < L - 1) {
                lv.has_up = true;
                lv.up = pk.conv("up_blocks." + std::to_string(i) + ".upsamplers.0.conv");
                // the sub-pixel form of `nearest x2 -> conv3x3` (4/9 of the MACs): bf16 engine, channel counts that fill K tiles
                if (sizeof(T) == 2 && lv.up.w && lv.up.ks == 3 && (4 * lv.up.cin) % 64 == 0 && lv.up.cout % 8 == 0) {
                    const RawParam* w = m.find(lv.up.name + ".weight");
                    lv.up_sp = m.new_packed((size_t)16 * lv.up.cout * lv.up.cin * sizeof(T), false);
                    if (!lv.up_sp || !w) pk.err = 4;
                    else if (launch_pack_conv_subpix<T>(static_cast<const float*>(w->data->p), lv.up_sp, lv.up.cout, lv.up.cin, st)) pk.err = 5;
                }
            }
            m.up.push_back(std::move(lv));
        }
        m.norm_out = pk.norm("conv_norm_out");
        m.conv_out = pk.conv("conv_out");
    } else {
        m.ce.clear();
        m.ce_stride.clear();
        // channel counts between the layers padded to the GEMM's K quantum (64): every layer but the 3-channel first one runs
        // through the implicit-GEMM conv kernels (the generic direct kernel needed 290 ms for a [16,3,512,512] condition batch)
        const int cq = 64;
        m.ce.push_back(pk.conv_padded("controlnet_cond_embedding.conv_in", false, true, cq));
        m.ce_stride.push_back(1);
        int nb = 0;
        while (m.find("controlnet_cond_embedding.blocks." + std::to_string(nb) + ".weight")) ++nb;
        for (int k = 0; k < nb; ++k) {
            m.ce.push_back(pk.conv_padded("controlnet_cond_embedding.blocks." + std::to_string(k), true, true, cq));
            m.ce_stride.push_back(k % 2 ? 2 : 1);
        }
        m.ce.push_back(pk.conv_padded("controlnet_cond_embedding.conv_out", true, false, cq));
        m.ce_stride.push_back(1);
        m.cn_down.clear();
        for (int k = 0; k < m.num_skips(); ++k) m.cn_down.push_back(pk.linear({"controlnet_down_blocks." + std::to_string(k)}));
        m.cn_mid = pk.linear({"controlnet_mid_block"});
    }
    if (pk.err) return pk.err;  // e.g. "missing parameter: <key>" (message already set)
    // all time_emb_proj linears as ONE [sum C][temb] matrix: a single weight-streaming launch per step
    {
        const int temb = 4 * c.block_out_channels[0];
        LinW tp;
        tp.n = m.tproj_total;
        tp.k = temb;
        tp.w = m.new_packed((size_t)tp.n * temb * sizeof(T), false);
        float* bias = static_cast<float*>(m.new_packed((size_t)tp.n * sizeof(float), true));
        if (!tp.w || !bias) return 4;
        int row = 0;
        for (auto& mod : m.temb_mods) {
            const RawParam* w = pk.need(mod + ".weight");
            const RawParam* b = pk.need(mod + ".bias");
            if (!w || !b) break;
            const int n = (int)w->shape[0];
            if (launch_pack_rows<T>(static_cast<const float*>(w->data->p), n, temb, tp.w, temb, row, 0, 0, 0, 1.0f, st)) pk.err = 5;
            MRISR_CHECK_HIP(hipMemcpyAsync(bias + row, b->data->p, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
            row += n;
        }
        tp.b = bias;
        m.tproj = tp;
    }
    if (pk.err) return pk.err;
    MRISR_CHECK_HIP(hipStreamSynchronize(st));
    m.finalized = true;
    if (!m.repacking) m.ws_key = "";  // force workspace re-plan (a re-pack keeps every geometry: only the caches below are stale)
    m.ctx_valid = false;
    m.cond_valid = false;
    return 0;
}

int Model::repack(hipStream_t st) {
    MRISR_REQUIRE(finalized, "re-pack of a model that was never finalized");
    repacking = true;
    repack_cursor = 0;
    const int rc = finalize(st);
    repacking = false;
    return rc;
}

int Model::finalize(hipStream_t st) {
    TRY(init_zero_page());
    if (cfg.compute_dtype == MRISR_F32) return finalize_t<float>(*this, st);
    return finalize_t<bf16>(*this, st);
}

int Model::num_skips() const {
    int n = 1;
    for (int i = 0; i < cfg.num_levels; ++i) n += cfg.layers_per_block + (i < cfg.num_levels - 1 ? 1 : 0);
    return n;
}
int Model::num_transformer_blocks() const {
    int n = 1;  // mid
    for (int i = 0; i < cfg.num_levels; ++i)
        if (cfg.attn_levels[i]) n += cfg.layers_per_block + (is_controlnet ? 0 : cfg.layers_per_block + 1);
    return n;
}
int Model::skip_shape(int k, int B, int h, int w, int64_t shape[4]) const {
    std::vector<std::pair<int, int>> s;  // (channels, level)
    s.push_back({cfg.block_out_channels[0], 0});
    for (int i = 0; i < cfg.num_levels; ++i) {
        for (int j = 0; j < cfg.layers_per_block; ++j) s.push_back({cfg.block_out_channels[i], i});
        if (i < cfg.num_levels - 1) s.push_back({cfg.block_out_channels[i], i + 1});
    }
    s.push_back({cfg.block_out_channels[cfg.num_levels - 1], cfg.num_levels - 1});  // mid
    MRISR_REQUIRE(k >= 0 && k < (int)s.size(), "skip index");
    shape[0] = B;
    shape[1] = s[k].first;
    shape[2] = h >> s[k].second;
    shape[3] = w >> s[k].second;
    return 0;
}
// x of decoder stage q = n - 1 - depth (up block q / (layers + 1), resnet q % (layers + 1)): the previous stage's output - the block's own
// width, or for the block's first resnet the width of the block below it, after the upsampler - at the resolution of the skip it meets
int Model::cache_shape(int depth, int B, int h, int w, int64_t shape[4]) const {
    const int n = num_skips(), per = cfg.layers_per_block + 1;
    MRISR_REQUIRE(depth >= 1 && depth <= n - 1, "cache depth must lie in 1 .. num_skips - 1");
    const int q = n - 1 - depth, j = q % per, lvl = cfg.num_levels - 1 - q / per;
    shape[0] = B;
    shape[1] = cfg.block_out_channels[j ? lvl : std::min(lvl + 1, cfg.num_levels - 1)];
    shape[2] = h >> lvl;
    shape[3] = w >> lvl;
    return 0;
}

// ================================================================================================
// workspace planning
// ================================================================================================
const HeadBuf& Model::head_buf(int N, int C) const {
    for (auto& h : heads)
        if (h.N == N && h.H * h.hd == C) return h;
    return heads.front();  // unreachable after planning
}
const HeadBuf& Model::head_buf_for_C(int C) const {
    for (auto& h : heads)
        if (h.H * h.hd == C) return h;
    return heads.front();
}

template <typename T>
static int dry_forward(Model& m, int B, int h, int w, int L, bool with_context, hipStream_t st);

template <typename T>
static int plan_t(Model& m, int B, int h, int w, int L, hipStream_t st) {
    const mrisr_unet_cfg& c = m.cfg;
    constexpr int BK = 128 / (int)sizeof(T);
    const bool flash = c.flash_attention && sizeof(T) == 2;
    ++m.ws_gen;
    m.heads.clear();
    m.ws_B = B; m.ws_h = h; m.ws_w = w; m.ctx_len = L;
    m.ctx_pad = round_up(L, 64);
    size_t persist = 0;
    auto carve = [&](size_t bytes) { size_t o = persist; persist = (persist + bytes + 255) & ~(size_t)255; return o; };
    // one (q, k, v^T) head-buffer set per distinct (tokens, channels): levels with attention + the mid block
    std::vector<std::pair<int, int>> keys;
    for (int i = 0; i < c.num_levels; ++i)
        if (c.attn_levels[i]) keys.push_back({(h >> i) * (w >> i), c.block_out_channels[i]});
    keys.push_back({(h >> (c.num_levels - 1)) * (w >> (c.num_levels - 1)), c.block_out_channels[c.num_levels - 1]});
    std::vector<size_t> offs;
    for (auto& kc : keys) {
        bool dup = false;
        for (auto& hb : m.heads) dup |= (hb.N == kc.first && hb.H * hb.hd == kc.second);
        if (dup) continue;
        HeadBuf hb;
        hb.B = B; hb.H = c.num_heads; hb.N = kc.first; hb.hd = kc.second / c.num_heads;
        hb.npad = round_up(hb.N, 64);
        hb.dpad = round_up(hb.hd, flash ? 32 : BK);
        const size_t qk = (size_t)B * hb.H * hb.npad * hb.dpad * sizeof(T);
        offs.push_back(carve(qk)); offs.push_back(carve(qk)); offs.push_back(carve(qk));
        m.heads.push_back(hb);
    }
    // cross-attention caches per transformer block
    std::vector<XfW*> xfs;
    for (auto& lv : m.down) for (auto& x : lv.xf) xfs.push_back(&x);
    xfs.push_back(&m.mid_xf);
    for (auto& lv : m.up) for (auto& x : lv.xf) xfs.push_back(&x);
    std::vector<size_t> xoffs;
    for (size_t i = 0; i < xfs.size(); ++i) xfs[i]->index = (int)i;  // forward order: the block's bit in PagState::mask
    for (XfW* x : xfs) {
        const HeadBuf& hb = m.head_buf_for_C(x->C);
        const size_t kb = (size_t)B * hb.H * m.ctx_pad * hb.dpad * sizeof(T);
        xoffs.push_back(carve(kb)); xoffs.push_back(carve(kb));
        xoffs.push_back(x->q2p ? carve(xattn_tail_kv_bytes(B)) : (size_t)0);
    }
    const size_t ctx_off = carve((size_t)B * L * c.cross_attention_dim * sizeof(T));
    m.cond_emb_bytes = (size_t)B * h * w * c.block_out_channels[0] * sizeof(T);
    const size_t cond_off = carve(m.cond_emb_bytes);
    TRY(m.persist.reserve(persist, false));
    MRISR_CHECK_HIP(hipMemsetAsync(m.persist.p, 0, persist, st));  // zero pads of the head buffers
    char* base = static_cast<char*>(m.persist.p);
    for (size_t i = 0; i < m.heads.size(); ++i) {
        m.heads[i].q = base + offs[3 * i];
        m.heads[i].k = base + offs[3 * i + 1];
        m.heads[i].vt = base + offs[3 * i + 2];
    }
    for (size_t i = 0; i < xfs.size(); ++i) {
        xfs[i]->kc = base + xoffs[3 * i];
        xfs[i]->vtc = base + xoffs[3 * i + 1];
        xfs[i]->kvp = xfs[i]->q2p ? base + xoffs[3 * i + 2] : nullptr;
    }
    m.ctx_rows = base + ctx_off;
    m.cond_emb = base + cond_off;
    m.ctx_valid = false;
    m.cond_valid = false;
    // dry pass -> exact arena size
    const int rc = dry_forward<T>(m, B, h, w, L, true, st);
    m.ctx_valid = false;
    m.cond_valid = false;
    if (rc) return rc;
    TRY(m.arena.buf.reserve(m.arena.peak + 4096, false));
    m.arena.reset();
    return 0;
}

// The forward without a launch, on B rows of h x w: leaves the arena's peak in m.arena.peak and plans (bf16: tunes) every GEMM of that
// shape.  with_context: the context projections and the condition embedding are part of the pass (a plan); without, they count as cached
// (a row window).  The worst case either way: ControlNet residuals and adapter features present.
template <typename T>
static int dry_forward(Model& m, int B, int h, int w, int L, bool with_context, hipStream_t st) {
    const mrisr_unet_cfg& c = m.cfg;
    m.arena.dry = true;
    m.arena.reset();
    m.arena.peak = 0;
    Runner<T> r(m, st, true);
    mrisr_tensor sample{}; sample.ndim = 4; sample.dtype = MRISR_F32;
    sample.shape[0] = B; sample.shape[1] = c.in_channels; sample.shape[2] = h; sample.shape[3] = w;
    mrisr_tensor ehs{}; ehs.ndim = 3; ehs.dtype = MRISR_F32; ehs.shape[0] = B; ehs.shape[1] = L; ehs.shape[2] = c.cross_attention_dim;
    const mrisr_tensor* pe = with_context ? &ehs : nullptr;
    int rc;
    const int ns = m.num_skips();
    std::vector<mrisr_tensor> res(ns + 1);
    for (int k = 0; k <= ns; ++k) {
        res[k] = mrisr_tensor{};
        res[k].ndim = 4; res[k].dtype = MRISR_F32; res[k].layout = MRISR_NCHW;
        m.skip_shape(k, B, h, w, res[k].shape);
    }
    if (!m.is_controlnet) {
        mrisr_tensor out = sample; out.shape[1] = c.out_channels;
        // worst case: ControlNet residuals + adapter features present
        std::vector<mrisr_tensor> intra(c.num_levels);
        for (int i = 0; i < c.num_levels; ++i) {
            intra[i] = res[0];
            intra[i].shape[1] = c.block_out_channels[i]; intra[i].shape[2] = h >> i; intra[i].shape[3] = w >> i;
        }
        rc = r.unet_forward(sample, nullptr, 0, pe, res.data(), ns, &res[ns], intra.data(), c.num_levels, out);
        if (!rc) rc = r.unet_forward(sample, nullptr, 1, pe, res.data(), ns, &res[ns], intra.data(), c.num_levels, out);
    } else {
        mrisr_tensor cond = sample; cond.shape[1] = c.cond_channels; cond.shape[2] = 8 * h; cond.shape[3] = 8 * w;
        rc = r.controlnet_forward(sample, nullptr, 0, pe, with_context ? &cond : nullptr, 1.0f, res.data(), ns, &res[ns]);
    }
    m.arena.dry = false;
    return rc;
}

int g_plan_salt = 0;

int Model::ensure_workspace(int B, int h, int w, int L, hipStream_t st) {
    MRISR_REQUIRE(finalized, "call mrisr_model_finalize first");
    const int div = 1 << (cfg.num_levels - 1);
    MRISR_REQUIRE(h % div == 0 && w % div == 0, "latent size must be divisible by 2^(levels-1)");
    char key[256];
    // (plan salt: the debug toggles that change WHAT the forward allocates - mrisr_debug_gn_slabs - bump it, so that the next forward re-plans)
    // (perturbed-attention guidance: the attention launches of an applied block cover fewer samples - other shapes to plan)
    snprintf(key, sizeof(key), "%d,%d,%d,%d,%d,s%d,p%x:%d:%d", B, h, w, L, keep ? 1 : 0, g_plan_salt, pag.on() ? pag.mask : 0u,
             pag.on() ? pag.first : 0, pag.on() ? pag.count : 0);
    if (freeu.on) {  // FreeU: six more launches in the decoder, their four scalars taken by value - or read from a sampler's schedule table
        const size_t n = strlen(key);
        if (freeu.sched) snprintf(key + n, sizeof(key) - n, ",fT");
        else snprintf(key + n, sizeof(key) - n, ",f%a:%a:%a:%a", (double)freeu.s[0], (double)freeu.s[1], (double)freeu.b[0], (double)freeu.b[1]);
    }
    if (cond.on) {  // a run with a conditioning table: no import copies of the residuals (UNet), no staged outputs (ControlNet)
        const size_t n = strlen(key);
        snprintf(key + n, sizeof(key) - n, cond.guess ? ",cG%d:%d" : ",cT%d:%d", cond.row_lo, cond.row_hi);
    }
    if (ws_key == key) return 0;
    int rc = cfg.compute_dtype == MRISR_F32 ? plan_t<float>(*this, B, h, w, L, st) : plan_t<bf16>(*this, B, h, w, L, st);
    if (rc) return rc;
    ws_key = key;
    return 0;
}

// A window of `rows` rows of the planned batch: one dry pass per (workspace generation, rows).  It plans every GEMM of that shape - the
// bf16 engine times its candidates there, which must never happen inside a stream capture - and measures the arena's peak.  Most shapes
// need less than the full batch does, but a smaller M can make the planner split K where the full batch does not, and the slabs of a split
// are not bounded by the full batch's allocations: so the peak is measured, not assumed, and an arena that is too small is replaced by a
// larger one.  That moves its base address, so ws_gen is bumped - graphs that baked the old one in are captured again - and nothing else
// changes: the persistent buffers, ws_key and every planned shape stay.  The arena's own bound check holds in any case.
int Model::check_window(int rows, hipStream_t st) {
    MRISR_REQUIRE(finalized && !ws_key.empty() && ws_B > 0, "row window: no planned workspace (run a forward or set the context first)");
    MRISR_REQUIRE(rows > 0 && rows <= ws_B, "row window: more rows than the planned batch");
    MRISR_REQUIRE(!keep, "row window: not while a training forward is being recorded");
    if (win_gen != ws_gen) { win_sized.clear(); win_gen = ws_gen; }
    for (int r : win_sized) if (r == rows) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    MRISR_CHECK_HIP(hipStreamIsCapturing(st, &cs));
    MRISR_REQUIRE(cs == hipStreamCaptureStatusNone, "row window: a window of a new size must be sized before the stream is captured");
    const int lo0 = win_lo, n0 = win_n;
    const size_t off0 = arena.off, peak0 = arena.peak;
    win_lo = ws_B - rows; win_n = rows;
    const int rc = cfg.compute_dtype == MRISR_F32 ? dry_forward<float>(*this, rows, ws_h, ws_w, ctx_len, false, st)
                                                  : dry_forward<bf16>(*this, rows, ws_h, ws_w, ctx_len, false, st);
    const size_t need = arena.peak + 4096;
    win_lo = lo0; win_n = n0;
    arena.off = off0; arena.peak = std::max(peak0, arena.peak);
    if (rc) return rc;
    if (need > arena.buf.bytes) {
        TRY(arena.buf.reserve(need, false));
        ++ws_gen;
        win_gen = ws_gen;
    }
    win_sized.push_back(rows);
    return 0;
}

// what a window forward needs instead of ensure_workspace (whose key carries the batch, the PAG state and the conditioning row range, none of
// which a window changes): a planned workspace of the same h, w, L whose batch contains the window.  Leaves win_lo / win_n set
int Model::enter_window(const RowWindow& rows, int B, int h, int w, int L, hipStream_t st) {
    MRISR_REQUIRE(finalized && !ws_key.empty(), "row window: no planned workspace (run a forward or set the context first)");
    MRISR_REQUIRE(rows.lo >= 0 && rows.lo < rows.hi && rows.hi <= ws_B, "row window: [lo, hi) must lie inside the planned batch");
    MRISR_REQUIRE(B == rows.hi - rows.lo, "row window: the sample must carry hi - lo rows");
    MRISR_REQUIRE(h == ws_h && w == ws_w && L == ctx_len, "row window: h, w and the context length must be the planned ones");
    MRISR_REQUIRE(ctx_valid && (!is_controlnet || cond_valid), "row window: the context (and the condition image) must be cached for the full batch");
    MRISR_REQUIRE(!pag.on() || rows.lo >= pag.first + pag.count || rows.hi <= pag.first, "row window: a window never contains perturbed rows");
    if (cond.on && !is_controlnet)
        MRISR_REQUIRE(cond.row_hi == 0 || (cond.row_lo == rows.lo && cond.row_hi == rows.hi),
                      "row window: the conditioning row range must be the window");
    TRY(check_window(B, st));
    win_lo = rows.lo; win_n = B;
    return 0;
}

static int check_sample(const Model& m, const mrisr_tensor* s) {
    MRISR_REQUIRE(s && s->ndim == 4 && s->shape[1] == m.cfg.in_channels, "sample must be [B, in_channels, h, w]");
    return 0;
}

int Model::build_tproj_table(const long long* ts_dev, int rows, float* scratch, float* table, hipStream_t st) {
    MRISR_REQUIRE(finalized && ts_dev && scratch && table && rows > 0, "time-embedding table: operands");
    if (cfg.compute_dtype == MRISR_F32) {
        Runner<float> r(*this, st, false);
        return r.time_embed_table(ts_dev, rows, scratch, table);
    }
    Runner<bf16> r(*this, st, false);
    return r.time_embed_table(ts_dev, rows, scratch, table);
}

int Model::forward_unet(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                        const mrisr_tensor* down_res, int n_down, const mrisr_tensor* mid_res,
                        const mrisr_tensor* intrablock, int n_intra, mrisr_tensor* out, hipStream_t st, const UNetCache* cache,
                        const RowWindow* rows) {
    MRISR_REQUIRE(!is_controlnet, "not a UNet handle");
    TRY(check_sample(*this, sample));
    MRISR_REQUIRE(timestep && timestep->dtype == MRISR_I64 && timestep->ndim <= 1, "timestep: device int64, 0-dim or [B]");
    MRISR_REQUIRE(out, "out tensor");
    const int B = (int)sample->shape[0], h = (int)sample->shape[2], w = (int)sample->shape[3];
    const int L = ehs ? (int)ehs->shape[1] : ctx_len;
    MRISR_REQUIRE(L > 0, "no encoder_hidden_states given and none cached");
    if (rows) {  // a window never contains perturbed rows, reads the cached context and runs the whole network
        MRISR_REQUIRE(!ehs, "row window: the context is the cached one (encoder_hidden_states must be null)");
        MRISR_REQUIRE(!cache || cache->mode == CACHE_NONE, "row window: not together with a feature cache");
    }
    if (pag.on()) {  // before the plan: nothing is launched for a state this batch cannot honour
        MRISR_REQUIRE(rows || pag.first + pag.count <= B, "perturbed-attention guidance: the perturbed samples lie outside the batch");
        MRISR_REQUIRE(!cache || cache->mode == CACHE_NONE, "perturbed-attention guidance together with a feature cache is not supported");
        MRISR_REQUIRE(!keep, "perturbed-attention guidance: not while a training forward is being recorded");
    }
    if (freeu.on) {  // likewise before the plan
        MRISR_REQUIRE(!cache || cache->mode == CACHE_NONE, "FreeU together with a feature cache is not supported");
        MRISR_REQUIRE(!keep, "FreeU: not while a training forward is being recorded");
    }
    if (cond.on) {  // likewise before the plan
        MRISR_REQUIRE(!keep, "conditioning table: not while a training forward is being recorded");
        MRISR_REQUIRE(cond.table && cond.step, "conditioning table: no table or step counter");
        MRISR_REQUIRE(rows || cond.row_hi == 0 || (cond.row_lo >= 0 && cond.row_lo < cond.row_hi && cond.row_hi <= B),
                      "conditioning table: the row range lies outside the batch");
    }
    struct WinGuard {  // win_lo / win_n are this call's: cleared on every exit path
        Model* m;
        ~WinGuard() { m->win_lo = m->win_n = 0; }
    } wguard{this};
    if (rows) TRY(enter_window(*rows, B, h, w, L, st));
    else TRY(ensure_workspace(B, h, w, L, st));
    const int t_scalar = timestep->ndim == 0 || timestep->shape[0] == 1;
    MRISR_REQUIRE(t_scalar || timestep->shape[0] == B, "timestep length");
    const long long* t = static_cast<const long long*>(timestep->data);
    const UNetCache fc = cache ? *cache : UNetCache();
    if (fc.mode != CACHE_NONE) {
        MRISR_REQUIRE(fc.mode == CACHE_STORE || fc.mode == CACHE_USE, "feature cache mode");
        MRISR_REQUIRE(fc.depth >= 1 && fc.depth <= num_skips() - 1, "cache depth must lie in 1 .. num_skips - 1");
        MRISR_REQUIRE(fc.p, "feature cache: null buffer");
        MRISR_REQUIRE(n_down == 0 && !mid_res, "a feature cache together with ControlNet residuals is not supported");
    }
    if (cfg.compute_dtype == MRISR_F32) {
        Runner<float> r(*this, st, false);
        return r.unet_forward(*sample, t, t_scalar, ehs, down_res, n_down, mid_res, intrablock, n_intra, *out, fc);
    }
    Runner<bf16> r(*this, st, false);
    return r.unet_forward(*sample, t, t_scalar, ehs, down_res, n_down, mid_res, intrablock, n_intra, *out, fc);
}

int Model::forward_controlnet(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                              const mrisr_tensor* cond, float scale, mrisr_tensor* down_out, int n_down,
                              mrisr_tensor* mid_out, hipStream_t st, const RowWindow* rows) {
    MRISR_REQUIRE(is_controlnet, "not a ControlNet handle");
    TRY(check_sample(*this, sample));
    MRISR_REQUIRE(timestep && timestep->dtype == MRISR_I64 && timestep->ndim <= 1, "timestep: device int64, 0-dim or [B]");
    const int B = (int)sample->shape[0], h = (int)sample->shape[2], w = (int)sample->shape[3];
    const int L = ehs ? (int)ehs->shape[1] : ctx_len;
    MRISR_REQUIRE(L > 0, "no encoder_hidden_states given and none cached");
    if (cond) MRISR_REQUIRE(cond->ndim == 4 && cond->shape[2] == 8 * h && cond->shape[3] == 8 * w, "controlnet_cond must be [B,3,8h,8w]");
    if (this->cond.on) MRISR_REQUIRE(!keep, "conditioning table: not while a training forward is being recorded");
    if (rows) MRISR_REQUIRE(!ehs && !cond, "row window: the context and the condition image are the cached ones (both must be null)");
    struct WinGuard {
        Model* m;
        ~WinGuard() { m->win_lo = m->win_n = 0; }
    } wguard{this};
    if (rows) TRY(enter_window(*rows, B, h, w, L, st));
    else TRY(ensure_workspace(B, h, w, L, st));
    const int t_scalar = timestep->ndim == 0 || timestep->shape[0] == 1;
    const long long* t = static_cast<const long long*>(timestep->data);
    if (cfg.compute_dtype == MRISR_F32) {
        Runner<float> r(*this, st, false);
        return r.controlnet_forward(*sample, t, t_scalar, ehs, cond, scale, down_out, n_down, mid_out);
    }
    Runner<bf16> r(*this, st, false);
    return r.controlnet_forward(*sample, t, t_scalar, ehs, cond, scale, down_out, n_down, mid_out);
}

int Model::set_context(const mrisr_tensor* ehs, int B, int h, int w, hipStream_t st) {
    MRISR_REQUIRE(ehs && ehs->ndim == 3, "encoder_hidden_states must be [B, L, D]");
    TRY(ensure_workspace(B, h, w, (int)ehs->shape[1], st));
    arena.reset();
    if (cfg.compute_dtype == MRISR_F32) {
        Runner<float> r(*this, st, false);
        return r.set_context(*ehs);
    }
    Runner<bf16> r(*this, st, false);
    return r.set_context(*ehs);
}

int Model::set_cond(const mrisr_tensor* cond, int L, hipStream_t st) {
    MRISR_REQUIRE(is_controlnet && cond && cond->ndim == 4, "controlnet_cond must be [B,3,8h,8w]");
    TRY(ensure_workspace((int)cond->shape[0], (int)cond->shape[2] / 8, (int)cond->shape[3] / 8, L, st));
    arena.reset();
    if (cfg.compute_dtype == MRISR_F32) {
        Runner<float> r(*this, st, false);
        return r.set_cond(*cond);
    }
    Runner<bf16> r(*this, st, false);
    return r.set_cond(*cond);
}

}  // namespace mrisr
