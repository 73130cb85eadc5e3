// StepPlan: everything the launches of one captured sampler step take by value or by pointer (sampler.hip: step_body reads this struct
// and nothing else).  The step graph of a sampler is reused exactly when the plan of the new run equals the plan it was captured from.
// Plain C++ with no HIP in it, so that the host check (tools/step_plan_check.cpp) compiles it with the host compiler alone.
#pragma once
#include <cstring>
#include <type_traits>

namespace mrisr {

constexpr int PLAN_MAX_RES = 32;    // ControlNet residuals: the down residuals, then the mid residual
constexpr int PLAN_MAX_INTRA = 8;   // adapter features

// Why a new field cannot be missed: equality is memcmp over the whole struct, so there is no per-field list to extend.  That is sound
// because (a) a plan starts as all-zero bytes (new_step_plan) and only then gets its fields, so unused array slots compare equal, and
// (b) the struct has no padding bytes: every member is a 4- or 8-byte scalar or an array of such, the 8-byte ones first, and -Wpadded is
// an error for the two definitions below - a new member that opens a hole does not compile.  Floats compare by their bits (-0 != +0:
// one capture more, never a stale graph).
#pragma GCC diagnostic push
#pragma GCC diagnostic error "-Wpadded"
struct PlanTensor {  // a 4-D tensor in the model's compute dtype, NHWC
    const void* data;
    long long shape[4];
};
struct StepPlan {
    // ---- device pointers ----
    float* x;             // the caller's latents [B]
    const float* lr;      // LR anchor or null
    const float* noise;   // step-noise slabs or null
    float* d_eps;         // the forward's output on the canvas [K B]
    float* d_x2;          // K > 1: the [K B] staging buffer the forwards read
    float* d_xt;          // tiled: the tile batch in ...
    float* d_et;          // ... and out
    const int* tile_oy;   // tiled: the uploaded table (d_tiles) - tile origins per axis ...
    const int* tile_ox;
    const float* tile_nwy;  // ... and the normalised window tables
    const float* tile_nwx;
    float* hist;          // multistep: the history ring
    float* xc;            // UniPC: the previous corrected state
    void* d_cache;        // feature cache
    const float* d_coef;
    int* d_step;
    long long* d_curt;
    const long long* d_ts;
    const float* d_sched;  // per-step schedule table [n_steps][8] = {g, s, phi, freeu s1, s2, b1, b2, 0}, or null: the scalars below rule
    const float* d_cond;   // conditioning table [n_steps][4] = {c, a, 0, 0}, or null: every residual at full strength
    const float* d_cons;   // consistency table [n_steps][4] = {w, alpha, beta, sigma}, or null: no consistency launch
    const float* cons_ref;    // ... its reference [B] and its noise slabs [n_steps][B] or null
    const float* cons_noise;
    // ---- model state the forwards bake in ----
    unsigned long long ws_gen_unet, ws_gen_cnet;  // workspace generations: persist / arena base addresses
    const float* tproj_unet;                      // per-run time-embedding tables (null: computed per step)
    const float* tproj_cnet;
    // ---- tensors ----
    PlanTensor res[PLAN_MAX_RES];  // ControlNet -> UNet residuals: n_res down residuals, then the mid residual at [n_res]
    PlanTensor intra[PLAN_MAX_INTRA];  // adapter features, converted    // ---- step configuration ----
    int kind;            // mrisr_step_kind
    int K, pag;          // parts of the forward (1, 2, 3); whether part 0 is the perturbed one
    int B, T, C, h, w, fh, fw, L;  // canvas batch, tiles per row (1: not tiled), channels, canvas and forward geometry, context length
    int cnet;            // a ControlNet runs before the UNet
    int n_res, n_intra;
    float clip;
    float guidance_scale, guidance_rescale;
    float pag_scale;
    unsigned pag_mask;
    int order;           // multistep: solver order (the ring's slabs)
    int cached, cache_depth;
    int tile_h, tile_w, tile_oh, tile_ow, tile_window;  // the five tile numbers (0: off)
    int tile_ky, tile_kx, tile_vec4;                    // the grid of this canvas; whether the 16-byte path applies
    int freeu;           // 0: off; 1: the four scalars below by value; 2: read from d_sched (the scalars stay zero)
    float freeu_s[2], freeu_b[2];
    // with d_sched the VALUES of a schedule are not here (guidance_scale, guidance_rescale, pag_scale, freeu_s / freeu_b stay zero): only what
    // chooses kernels.  sched_phi: some row of the table has phi > 0 - the guided step is the rescale kernel.  sched_rows: the table's rows
    int sched_phi, sched_rows;
    // with d_cond the VALUES of the conditioning table are not here either.  cond_guess: guess mode (the per-residual weights; under
    // classifier-free guidance the ControlNet runs on the conditional rows only).  cnet_rows: the rows of the ControlNet's forward
    int cond_guess, cnet_rows;
    // with d_cons the VALUES of the consistency table are not here either: only the launch constants, the factor N and the filter
    int cons_factor, cons_filter;
    int first;           // the step the run starts at (the time-embedding table's row 0)
    // ---- policy, not baked in: these live in the uploaded rows; a change captures again because set_solver promises it ----
    int final_zero, lower_order_final;
    int n_disabled;
    int disabled[32];    // the disabled-corrector list (its first 32 entries)
    int cdt;             // compute dtype of the tensors above
};
#pragma GCC diagnostic pop
static_assert(std::is_trivially_copyable<StepPlan>::value, "StepPlan is compared and copied as bytes");

inline StepPlan new_step_plan() {
    StepPlan p;
    std::memset(&p, 0, sizeof(p));
    return p;
}
inline bool same_plan(const StepPlan& a, const StepPlan& b) { return std::memcmp(&a, &b, sizeof(StepPlan)) == 0; }

}  // namespace mrisr
