/* mrisr_debug.h - test hooks and tuning tools exported by libmrisr.so.
 *
 * NOT part of the drop-in surface (include/mrisr.h): these are process-global switches used by the parity tests
 * (tests/test_gpu_*.py force split-K, a tile, an older code path, so that every kernel variant is exercised against
 * the oracle) and by the measurement tools under tools/ (tile sweeps, autotuner statistics).  A product caller never
 * needs them.  All are no-ops for correctness: every setting selects between implementations of the same arithmetic.
 */
#ifndef MRISR_DEBUG_H
#define MRISR_DEBUG_H
#ifdef __cplusplus
extern "C" {
#endif

/* GEMM planner overrides (0 restores the planner): a split-K factor for every GEMM that can be split; one kernel
 * configuration (a tile id) for every GEMM; a kernel of a specialised family (halo conv, 256-row halo conv, weight-stationary,
 * row-panel) wherever it is eligible.  The tile ids, their families and template parameters are the lines of the tile
 * registry in csrc/gemm.hip (TILES); nothing outside that file knows a tile number.  A forced tile that does not take a
 * launch's form is refused with the reason, except that f32 / 2 GiB operands, 2 x 2 / sub-pixel convs and splits on a family
 * without split-K move to the default tile of the family that takes them (gemm.hip: tile_for_launch), and that a launch with
 * a 1x1 tail leaves a forced tile that cannot carry it to the planner. */
void mrisr_debug_force_split(int splitk);
void mrisr_debug_force_tile(int tile);
void mrisr_debug_prefer_tile(int tile);
/* bit flags: 8 = rank-4 LoRA up-projection in the scalar epilogue instead of on the matrix cores; 16 = head-major outputs
 * stored straight from the accumulator layout instead of through LDS; 2048 = every GEMM workgroup fills its LDS allocation with
 * 0xFF bytes (NaN) before its first LDS-DMA, so that a read that runs ahead of its DMA cannot return plausible stale data;
 * 64 = the plain staged epilogue of the tiled and halo GEMM kernels (alpha * acc + bias [+ time row] into the LDS tile) runs
 * through the generic per-fragment epilogue, as it did, instead of its own few lines (the same operations: bit-identical outputs) */
void mrisr_debug_gemm_flags(int flags);
/* probe (tools/probes/bl_stamps.py): dev_buf = 256 slots of (8 + 8 * 1024) u64.  Every eager launch of tile id `tile` on the tiled
 * 2-stage kernel or the 4-wave halo kernel takes the next slot (the counted-ring tiles carry no stamps; launches past the last slot are not
 * stamped): 8 words describing the launch (M, N, K, workgroups, 1 residual | 2 in-kernel LoRA | 4 conv | 8 1x1 tail, split-K, gemm flags, 1), then per workgroup (the
 * first 1024) 8 clock stamps (shader-clock ticks) of wave 0: entry, head finished and stage-0 DMA all issued, first stage landed, K loop done, bias / LoRA
 * ready, tile staged in LDS, residual loaded (written by the staged row copy-out only: 0 for head-major and unstaged outputs), last store
 * issued.  Workgroups past the first 1024 write nothing.  NULL (default) = off; each call restarts at slot 0 */
void mrisr_debug_gemm_stamps(void* dev_buf, int tile);
/* M tiles per group of the tiled kernels' tile order for every later launch; > 0: this value, NOT clamped to the launch's M tiles (a group
 * larger than the grid, short last groups); 0 (default): MRISR_GROUP_M, else 8, clamped.  The order changes no output bit */
void mrisr_debug_group_m(int group_m);
/* 1: mrisr_op_conv3x3 with stride 2 (even H, W) pads the low side with 0 instead of 1 - the (0,1,0,1) padding of the VAE encoder's
 * down-samplers - so that the op reaches that form of the tiled kernels' gather; 0 (default): pad 1 */
void mrisr_debug_op_conv_pad0(int on);
/* cost-model efficiency of one tile id (only used when the autotuner is off) */
void mrisr_debug_set_tile_eff(int tile, double eff);
/* override one entry of the in-process tile table (key as in the MRISR_TUNE_CACHE file) */
void mrisr_debug_set_tuned(const char* key, int tile, int splitk);
/* 0: two-kernel GroupNorm everywhere; 1: the one-pass kernel where the geometry allows (default) */
void mrisr_debug_gn_fused(int on);

/* plan-time autotuner: number of signatures tuned and the time spent; free its scratch operands */
int mrisr_autotune_stats(int* shapes, double* ms);
void mrisr_autotune_release(void);

/* micro-benchmark of one GEMM / conv signature on random operands (tools/gemm_sweep.py): average ms over `iters` */
int mrisr_bench_gemm(int M, int N, int K, int conv, int B, int H, int W, int stride, int ups, int c1, int tile, int splitk,
                     int iters, float* ms_out);

/* split-K: 1 the last split of a tile to arrive reduces inside the GEMM kernel, 0 the separate reduce kernel,
 * -1 (default) as MRISR_SK_INKERNEL says (unset: the reduce kernel - measured no slower, see gemm.hip sk_counters_for) */
void mrisr_debug_sk_inkernel(int on);

/* the sub-pixel form of the decoder's `nearest x2 -> conv3x3` layers (bf16 inference): -1 default (MRISR_SUBPIX, 2048 low-resolution
 * rows), 0 off (the literal up-sampled conv), n > 0: from n rows on */
void mrisr_debug_subpix(int min_rows);

/* fused sampler: time embeddings of all steps of a run computed once (a table, one row copied per step) instead of sinusoid + three GEMVs in
 * every step: -1 default (MRISR_TEMB_TABLE, on), 0 per step, 1 on */
void mrisr_debug_temb_table(int on);

/* the transformer's proj_out + outer residual as a continuation of the fused feed-forward kernel (C = 320): -1 default (MRISR_MLP_PROJ, on),
 * 0 its own launch, 1 on */
void mrisr_debug_mlp_proj(int on);

/* split-K conv whose only consumer is a GroupNorm: -1 default (MRISR_GN_SLABS, on) the GroupNorm kernel sums the f32 slabs itself
 * (one launch instead of splitk_reduce + GroupNorm), 0 the two launches, 1 on */
void mrisr_debug_gn_slabs(int on);

/* a resnet's 1x1 conv_shortcut as the last K steps of its conv2 (bf16 inference; one launch on a concatenated filter bank instead of
 * shortcut GEMM + conv2 with a residual): -1 default (MRISR_SC_FUSED, on), 0 the two launches, 1 on */
void mrisr_debug_sc_fused(int on);

/* a transformer block's ff.net.2 and the transformer's proj_out as ONE GEMM over K = [4C | C] (bf16 inference, C >= 640: the composed
 * weight [Wp W2 | Wp] built at finalize, sources the GEGLU output and the residual stream): -1 default (MRISR_FF_PROJ_FUSED, on),
 * 0 the two launches, 1 on */
void mrisr_debug_ff_proj_fused(int on);

/* the fused row-local middle of the C = 320 transformer blocks (csrc/xtail.hip: attn1.to_out + residual, LayerNorm2, attn2.to_q,
 * cross-attention, attn2.to_out + residual in one launch): -1 default (MRISR_XTAIL, on), 0 the four separate launches, 1 on */
void mrisr_debug_xattn_tail(int on);
/* probe: device buffer of (workgroups x 40) u64 that every launch of that kernel fills with clock stamps at its phase boundaries
 * (tools/probes/xtail_stamps.py); NULL (default) = off */
void mrisr_debug_xattn_tail_stamps(void* dev_buf);

/* micro-benchmark of the fused feed-forward kernel (tools/mlp_probe.py): M rows of width 320, random operands */
int mrisr_bench_mlp(int M, int hidden, int iters, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* MRISR_DEBUG_H */
