// Model object behind the opaque mrisr_model handle (UNet2DConditionModel or ControlNetModel).
#pragma once
#include "runtime.h"

namespace mrisr {

struct ResW {
    NormW n1, n2;
    ConvW c1, c2;
    bool has_sc = false;
    LinW sc;
    int temb_off = 0, cin = 0, cout = 0;
    // bf16 engine, has_sc: conv2 and the shortcut as ONE filter bank [cout][9 * cout + cin] (the shortcut's columns last) and the summed bias
    // b2 + b_sc - conv2 then runs the shortcut as a 1x1 tail of its K loop (runner.h::resnet); c2 / sc stay for the literal and training paths
    void* c2sc = nullptr;
    const float* b2sc = nullptr;
};
struct XfW {
    int C = 0;
    NormW norm, ln1, ln2, ln3;
    LinW proj_in, proj_out, qkv, out1, q2, kv2, out2, ff1, ff2;
    void* ff2p = nullptr;  // ff2.w with K permuted for the fused feed-forward kernel (bf16, C = 320 only)
    void* kc = nullptr;   // cached cross-attention K   [B*H][ctx_pad][dpad]
    void* vtc = nullptr;  // cached cross-attention V^T [B*H][dpad][ctx_pad]
    // fused row-local middle of the block (xtail.hip; bf16, C = 320): attn2.to_q / attn2.to_out weights with K permuted to the
    // accumulator order, and the prompt K / V as per-(image, head pair) LDS images (planned with kc / vtc, packed by set_context)
    void* q2p = nullptr;
    void* proj_outp = nullptr;  // proj_out.w K-permuted: the continuation of the fused feed-forward kernel
    void* out2p = nullptr;
    void* kvp = nullptr;
    // bf16 engine, blocks outside the fused feed-forward kernel (C >= 640): ff.net.2 and proj_out - two linear maps with only a residual add
    // between them - as ONE weight [C][4C + C] = [Wp W2 | Wp] (the product in f32 from the masters, rounded once; the last C columns the packed
    // proj_out.w) and the bias Wp b2 + bp: o = [ff | t] ffpo^T + bffpo + x is one GEMM (runner.h::transformer); ff2 / proj_out stay for the
    // literal and training paths
    void* ffpo = nullptr;
    const float* bffpo = nullptr;
    int index = -1;  // position among the handle's transformer blocks in forward order (down, mid, up): the block's bit in PagState::mask
};
struct Level {
    std::vector<ResW> res;
    std::vector<XfW> xf;
    bool has_down = false, has_up = false;
    ConvW down, up;
    void* up_sp = nullptr;  // bf16 inference: `up` as four 2 x 2 parity banks [4][cout][2][2][cin] (sub-pixel form, launch_pack_conv_subpix)
};
struct HeadBuf {  // head-major q / k / v^T staging for one (tokens, channels) geometry; pads stay zero
    int B = 0, H = 0, N = 0, hd = 0, npad = 0, dpad = 0;
    void* q = nullptr;
    void* k = nullptr;
    void* vt = nullptr;
};

const char* last_error_cstr();

// DeepCache-style feature cache of one UNet forward.  With n = num_skips() and 1 <= depth <= n - 1, decoder stage
// n - 1 - depth (the up-block resnet that consumes skip s_depth) reads x = the tensor `p` describes ([B, H, W, C] of Model::cache_shape,
// NHWC, compute dtype).  STORE: the ordinary forward, which also copies that x into p.  USE: the encoder stops after producing s_depth, no
// mid block runs, and the decoder starts at that stage from p.
enum { CACHE_NONE = 0, CACHE_STORE = 1, CACHE_USE = 2 };
struct UNetCache {
    int mode = CACHE_NONE;
    int depth = 0;
    void* p = nullptr;
};

// Perturbed-attention guidance: in the transformer blocks whose bit is set in `mask`, self-attention of samples
// [first, first + count) is the identity map - their attention output is their own value rows - and the other samples attend as usual.
// count == 0: off.  Part of the workspace key: the dry pass plans the attention launches of the remaining samples.
struct PagState {
    unsigned mask = 0;
    int first = 0, count = 0;
    bool on() const { return count > 0 && mask != 0; }
};

// FreeU (diffusers' enable_freeu): in every resnet stage of up block k in {0, 1} the first half of the hidden
// channels is scaled by b[k] and the skip tensor's lowest spatial frequencies by s[k], before the concat.  Part of the workspace key.
// sched / step: a sampler run with a per-step schedule points them at its table [n_steps][8] and its step counter for
// the duration of the run; the launches then read (s1, s2, b1, b2) from columns 3..6 of row *step and the key carries a marker instead
// of the four values.  Null outside such a run.
struct FreeUState {
    bool on = false;
    float s[2] = {1.f, 1.f}, b[2] = {1.f, 1.f};
    const float* sched = nullptr;
    const int* step = nullptr;
};

// Conditioning strength: a sampler run with a conditioning table sets this on its UNet and its ControlNet for the
// duration of the run (a guard clears it on every exit path).  Part of the workspace key.
// UNet: the ControlNet residuals (NHWC, compute dtype, read where the ControlNet wrote them) are added by launch_cond_add - the down
// residuals in one launch, the mid residual in a second - with f_k = w[k] * table[4 * (*step)] on rows [row_lo, row_hi) of the batch
// (row_hi == 0: every row); the adapter features by the same kernel, one launch each, with column 1 on every row.
// ControlNet: the output convolutions write straight into the caller's NHWC tensors (no export copy).
struct CondState {
    bool on = false;
    bool guess = false;
    const float* table = nullptr;  // [n_steps][4] = {c, a, 0, 0}
    const int* step = nullptr;
    int row_lo = 0, row_hi = 0;
    float w[32] = {};              // per residual, the mid residual after the down residuals (PLAN_MAX_RES entries)
};

// A forward on a row window [lo, hi) of the batch the workspace is planned for: `sample` (and every residual and
// feature) carries hi - lo rows, the persistent per-row buffers - the cross-attention K / V caches of every transformer block, the
// ControlNet's condition embedding - are read at row lo, and nothing is planned again: ws_gen and ws_key stay as they are.
struct RowWindow {
    int lo = 0, hi = 0;
};

struct Model {
    mrisr_unet_cfg cfg{};
    bool is_controlnet = false;
    std::map<std::string, RawParam> raw;
    float lora_scale = 1.0f;
    bool dora = false;  // DoRA handle (mrisr_model_set_dora): every adapted linear carries a magnitude vector
    bool finalized = false;
    PagState pag;       // mrisr_model_set_pag: honoured by every forward_unet until cleared
    FreeUState freeu;   // mrisr_model_set_freeu: honoured by every forward_unet until cleared
    CondState cond;     // set by a sampler run with a conditioning table, for that run only
    std::vector<std::unique_ptr<DevBuf>> packed;

    // packed modules
    ConvW conv_in, conv_out;
    NormW norm_out;
    LinW te1, te2, tproj;
    std::vector<std::string> temb_mods;
    int tproj_total = 0;
    std::vector<Level> down, up;
    ResW mid_r0, mid_r1;
    XfW mid_xf;
    std::vector<ConvW> ce;  // ControlNet condition embedding
    std::vector<int> ce_stride;
    std::vector<LinW> cn_down;
    LinW cn_mid;

    // workspace (planned per input geometry)
    Arena arena;
    DevBuf persist;
    std::string ws_key;
    unsigned long long ws_gen = 0;  // bumped whenever persist / arena are re-planned or reallocated: captured graphs that
                                    // baked the old addresses in must be re-captured (mrisr_sampler_run keys on it)
    int ws_B = 0, ws_h = 0, ws_w = 0, ctx_len = 0, ctx_pad = 0;
    std::vector<HeadBuf> heads;
    void* ctx_rows = nullptr;
    void* cond_emb = nullptr;
    size_t cond_emb_bytes = 0;
    bool ctx_valid = false, cond_valid = false;
    bool keep = false;  // training forward: never release arena temporaries (the backward reads them)
    // window forward (RowWindow): the rows of the planned batch this forward runs on, set for the duration of the call (win_n == 0: none);
    // the window sizes whose dry pass has run against workspace generation win_gen (check_window)
    int win_lo = 0, win_n = 0;
    std::vector<int> win_sized;
    unsigned long long win_gen = 0;
    int check_window(int rows, hipStream_t st);  // dry pass at `rows` rows: tunes its GEMMs, proves (or makes) the arena large enough
    int enter_window(const RowWindow& rows, int B, int h, int w, int L, hipStream_t st);
    // per-forward state
    float* tproj_out = nullptr;
    // fused sampler: the time embedding of EVERY step of the schedule computed once per run (they depend on the timestep only); the step then
    // copies row (*tproj_step - tproj_first) instead of running the sinusoid + three GEMVs (50 MB of weights per step).  Null outside a run.
    const float* tproj_table = nullptr;
    const int* tproj_step = nullptr;
    int tproj_first = 0;
    int build_tproj_table(const long long* ts_dev, int rows, float* scratch, float* table, hipStream_t st);
    float *te_s = nullptr, *te_y1 = nullptr, *te_emb = nullptr;  // the time-embedding MLP's activations of this forward (training reads them)
    float* d_tproj = nullptr;                                     // full-parameter training: d(loss)/d(tproj_out), [rows][tproj_total]
    int t_scalar = 1;

    int set_param(const char* key, const float* data, const int64_t* shape, int ndim, int is_device);
    int64_t num_params() const;
    const RawParam* find(const std::string& k) const;
    void* new_packed(size_t bytes, bool zero);
    int finalize(hipStream_t st);
    int num_skips() const;
    int num_transformer_blocks() const;
    int skip_shape(int k, int B, int h, int w, int64_t shape[4]) const;
    int cache_shape(int depth, int B, int h, int w, int64_t shape[4]) const;  // the cached decoder input of UNetCache: {B, C, H, W}
    const HeadBuf& head_buf(int N, int C) const;
    const HeadBuf& head_buf_for_C(int C) const;
    int ensure_workspace(int B, int h, int w, int L, hipStream_t st);
    int forward_unet(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                     const mrisr_tensor* down_res, int n_down, const mrisr_tensor* mid_res,
                     const mrisr_tensor* intrablock, int n_intra, mrisr_tensor* out, hipStream_t st, const UNetCache* cache = nullptr,
                     const RowWindow* rows = nullptr);
    int forward_controlnet(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                           const mrisr_tensor* cond, float scale, mrisr_tensor* down_out, int n_down,
                           mrisr_tensor* mid_out, hipStream_t st, const RowWindow* rows = nullptr);
    int set_context(const mrisr_tensor* ehs, int B, int h, int w, hipStream_t st);
    int set_cond(const mrisr_tensor* cond, int L, hipStream_t st);

    // ---- LoRA fine-tuning (train.hip) ----
    struct Trainable { std::string key; long long offset, numel; int rows, cols; int ndim = 2; long long shape[4] = {0, 0, 0, 0}; };  // (shape: 4-D conv adapters)
    std::vector<Trainable> trainables;   // lora_A / lora_B tensors in flat-vector order
    long long n_trainable = 0;
    float* theta = nullptr;              // caller-owned flat f32 parameter vector (bound)
    float* grad = nullptr;               // caller-owned flat f32 gradient vector (bound)
    bool train_ready = false;
    std::vector<mrisr_tensor> d_intra;   // optional outputs: gradients w.r.t. the T2I-Adapter features of the next train_step
    // ControlNet residuals of the next train_step (inputs) and the tensors their gradients are written to (outputs): 12 + mid
    std::vector<mrisr_tensor> tr_down, d_tr_down;
    mrisr_tensor tr_mid{}, d_tr_mid{};
    bool has_tr_mid = false;
    std::string train_ws_key;
    // ---- full-parameter training (ControlNet: every raw tensor is trainable; train.hip "full gradient" blocks) ----
    std::map<std::string, long long> full_off;   // raw key -> offset in the caller's flat f32 vectors
    std::vector<Trainable> full_trainables;      // every raw tensor, in key order (rows = shape[0], cols = the rest)
    std::vector<std::string> full_unsupported;   // tensors whose gradient this build leaves at zero (reported to the host)
    long long n_full = 0;
    float* full_theta = nullptr;                 // caller-owned flat parameters / gradients (bound by full_train_bind)
    float* full_grad = nullptr;
    std::shared_ptr<void> full_tape;             // the recorded forward of full_train_forward (a Trainer<T>), consumed by full_train_backward
    int full_train_prepare(hipStream_t st);
    int full_train_bind(float* theta_dev, float* grad_dev, int init_from_model, hipStream_t st);
    int full_train_refresh(hipStream_t st);      // copy theta back into the f32 masters and re-pack every weight
    int repack(hipStream_t st);                  // finalize again INTO the existing packed buffers (same parameter set, new values)
    bool repacking = false;
    size_t repack_cursor = 0;
    int controlnet_train_forward(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs, const mrisr_tensor* cond,
                                 float scale, mrisr_tensor* down_out, int n_down, mrisr_tensor* mid_out, hipStream_t st);
    int controlnet_train_backward(const mrisr_tensor* d_down, int n_down, const mrisr_tensor* d_mid, float scale, hipStream_t st);
    std::vector<LinW*> lora_linears();   // every LinW that carries adapters, fixed order
    std::vector<ConvW*> lora_convs();    // every resnet conv that carries an adapter: resnets in walk order, conv1 then conv2
    int train_prepare(hipStream_t st);   // dgrad weight copies + trainable layout (after finalize)
    int train_bind(float* theta_dev, float* grad_dev, hipStream_t st);
    int lora_refresh(hipStream_t st);    // re-pack the adapters from theta
    int train_plan(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs, const mrisr_tensor* intrablock,
                   int n_intra, const mrisr_tensor* target, float* loss_dev,
                   hipStream_t st);  // train_step's workspace planning alone (synchronises; never inside a capture)
    int train_step(const mrisr_tensor* sample, const mrisr_tensor* timestep, const mrisr_tensor* ehs,
                   const mrisr_tensor* intrablock, int n_intra, const mrisr_tensor* target, float* loss_dev,
                   mrisr_tensor* pred_out, hipStream_t st);
};

// ---- the T2I-Adapter inside the device training loop (adapter.hip; used by fit.hip) ----
struct AdapterFitInfo {
    int compute_dtype, cin, nums_rb, n_levels;
    int channels[4];
    long long n_trainable;
    float* theta;  // bound flat parameter / gradient vectors (null: not bound)
    float* grad;
};
int adapter_fit_info(const mrisr_adapter* a, AdapterFitInfo* out);
// dry forward + backward from u [B, cin, h, w] (stored NHWC, compute dtype), arena reserve, GEMM tuning: synchronises; a no-op while the
// geometry is planned.  Never inside a capture.
int adapter_fit_plan(mrisr_adapter* a, const mrisr_tensor* u, mrisr_tensor* feats, const mrisr_tensor* d_feats, int n_feats, hipStream_t st);
int adapter_fit_forward(mrisr_adapter* a, const mrisr_tensor* u, mrisr_tensor* feats, int n_feats, hipStream_t st);  // launches only
int adapter_fit_backward(mrisr_adapter* a, const mrisr_tensor* d_feats, int n_feats, hipStream_t st);               // adds into grad
int adapter_fit_repack(mrisr_adapter* a, hipStream_t st);  // forward and dgrad banks from theta (mrisr_adapter_train_refresh)
std::string adapter_fit_key(const mrisr_adapter* a);      // every address a capture of the calls above bakes in, plus the plan generation

}  // namespace mrisr
