// High-rank LoRA (r = 32 .. 128): the index arithmetic of the packed layout and of the lora_wgrad_hr kernel as plain
// host functions - no HIP in here, so tools/lora_hr_check.cpp runs them under the host sanitizers.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define MRISR_HD __host__ __device__
#else
#define MRISR_HD
#endif

namespace mrisr {

inline bool lora_rank_low(int r) { return r >= 4 && r <= 16 && r % 4 == 0; }
inline bool lora_rank_high(int r) { return r >= 32 && r <= 128 && r % 16 == 0; }

// K tile of the tiled GEMMs in elements: an adapter's columns are padded to whole tiles (launch_gemm: c1 % BK == 0)
inline int lora_hr_ktile(int elem_size) { return elem_size == 2 ? 64 : 32; }
inline int lora_hr_rp(int r, int elem_size) {
    const int kt = lora_hr_ktile(elem_size);
    return (r + kt - 1) / kt * kt;
}
inline int lora_hr_Rp(int r, int nmod, int elem_size) { return nmod * lora_hr_rp(r, elem_size); }
// first column of module j's (alpha / r) B block in a row of the [n][k + Rp] weight; module j's rows of loraA [Rp][k] start at j * rp
inline int lora_hr_wcol(int k, int j, int rp) { return k + j * rp; }

// lora_wgrad_hr (bf16): a workgroup owns HR_TC channels x HR_TQ columns of Q over one slab of rows
constexpr int HR_TC = 64, HR_TQ = 64, HR_STEP = 32, HR_MAX_SLABS = 256, HR_MIN_ROWS = 256;
struct LoraHrGeom {
    int tps = 0;    // channel tiles per section (mode 0: a tile never straddles two modules)
    int tiles = 0;  // channel tiles in all
    int qblk = 0;   // HR_TQ-column blocks of Q a channel tile meets: rp / 64 (dB, its own module's), nmod * rp / 64 (dA)
    int rows = 0;   // rows per slab, a multiple of HR_STEP
    int gz = 0;     // slabs
};
MRISR_HD inline LoraHrGeom lora_wgrad_hr_geom(int M, int C, int mode, int rp, int nmod, int secN) {
    LoraHrGeom g;
    if (mode == 0) {
        g.tps = (secN + HR_TC - 1) / HR_TC;
        g.tiles = nmod * g.tps;
        g.qblk = rp / HR_TQ;
    } else {
        g.tps = (C + HR_TC - 1) / HR_TC;
        g.tiles = g.tps;
        g.qblk = nmod * rp / HR_TQ;
    }
    int rows = (M + HR_MAX_SLABS - 1) / HR_MAX_SLABS;
    if (rows < HR_MIN_ROWS) rows = HR_MIN_ROWS;
    g.rows = (rows + HR_STEP - 1) / HR_STEP * HR_STEP;
    g.gz = (M + g.rows - 1) / g.rows;
    return g;
}
// first channel, channel limit and first Q column of block (tile, qb)
MRISR_HD inline void lora_wgrad_hr_tile(const LoraHrGeom& g, int mode, int C, int rp, int secN, int tile, int qb, int& c0, int& cend, int& qcol0) {
    if (mode == 0) {
        const int j = tile / g.tps;
        c0 = j * secN + (tile - j * g.tps) * HR_TC;
        cend = (j + 1) * secN;
        qcol0 = j * rp + qb * HR_TQ;
    } else {
        c0 = tile * HR_TC;
        cend = C;
        qcol0 = qb * HR_TQ;
    }
}
inline size_t lora_wgrad_hr_partial_floats(const LoraHrGeom& g) { return (size_t)g.gz * g.tiles * g.qblk * HR_TC * HR_TQ; }

}  // namespace mrisr
