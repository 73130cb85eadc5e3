// The launch head of the tiled (gemm_bl_kernel) and halo (gemm_halo_kernel) GEMMs: everything a workgroup needs before its first LDS-DMA,
// computed ONCE on the host and passed as the first 128 bytes (two 64-byte lines) of the kernel arguments, and the exact multiply-and-shift
// divisions that go with it.  No HIP here: the host fills it (launch_bl / launch_halo in gemm.hip), the kernels decode it with the inline
// functions below, and tools/gemm_head_check.cpp runs the same functions on the CPU against plain `/` and `%`.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRISR_GH_HD __host__ __device__ __forceinline__
#else
#define MRISR_GH_HD inline
#endif

namespace mrisr {

// ---- division by a launch constant -------------------------------------------------------------------------------------------
// q = x / d for every 0 <= x < 2^31 and 1 <= d < 2^31:  q = (x * mul) >> (31 + l)  with  l = ceil(log2 d),  mul = ceil(2^(31 + l) / d).
// (Granlund & Montgomery 1994, N = 31: 2^(31+l) <= mul * d <= 2^(31+l) + 2^l, and mul < 2^32 because d > 2^(l-1); d = 1 gives mul = 2^31.)
// Every dividend in the two kernels is a non-negative int, so the range is the whole admitted one.
struct MagicDiv {
    uint32_t mul;
    uint32_t l;  // 0 .. 31
};
inline MagicDiv magic_for(uint32_t d) {
    MagicDiv m{0x80000000u, 0u};
    if (d <= 1) return m;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    m.l = l;
    m.mul = (uint32_t)(((1ull << (31 + l)) + d - 1) / d);
    return m;
}
MRISR_GH_HD uint32_t magic_div(uint32_t x, uint32_t mul, uint32_t l) { return (uint32_t)(((uint64_t)x * mul) >> (31u + l)); }

// ---- the head ------------------------------------------------------------------------------------------------------------------
enum : uint32_t {
    GH_DBG_MASK = 0xFFFFu,   // mrisr_debug_gemm_flags, low 16 bits (the kernels' switches lie below 32768)
    GH_CONV = 1u << 16,
    GH_SUBPIX = 1u << 17,
    GH_ZSTUFF = 1u << 18,
    GH_UPS = 1u << 19,
    GH_A1 = 1u << 20,        // a second A source
    GH_TAIL = 1u << 21,      // a 1x1 tail (cs0 > 0)
    GH_STAMPED = 1u << 22,   // GemmArgs::stamps is set
    GH_BATCHED = 1u << 23,   // blockIdx.z > 0 exists: a_bs / w_bs are read from GemmArgs
};
enum { GH_SH_PG = 0, GH_SH_GM = 5, GH_SH_LAST = 10, GH_SH_HW = 15, GH_SH_WD = 20, GH_SH_PW = 25 };  // 5-bit fields of GemmHead::shifts

struct GemmHead {
    // line 0
    const void* w;        // operand pointers (batch 0)
    const void* a0;
    const void* a1;       // null: a0 with extent 0
    uint32_t ext_w, ext_a0, ext_a1;  // byte extents of the three buffer descriptors, clamped to 2^31 - 1
    uint32_t flags;       // GH_*
    uint32_t rows;        // tiled: M; halo: Hin
    uint32_t N;
    uint32_t wpitch;      // K * 2: bytes of a weight row (K tiles: wpitch >> 7)
    uint32_t lda0, lda1;  // A row pitches, elements
    uint32_t c0;
    // line 1
    uint32_t ntn, ntm;    // tiles along N and M
    uint32_t group_m;     // M tiles per group of the tile order (>= 1)
    uint32_t mul_pg, mul_gm, mul_last;  // / (group_m * ntn), / group_m, / (the short last group's size)
    uint32_t shifts;      // six 5-bit `l` values: GH_SH_*
    uint32_t per;         // K tiles (tiled) or 64-channel chunks (halo) per split
    uint32_t Ct;          // c0 + c1
    uint32_t pt_per_wg, pt_per_wave;  // pre-touch: 1-KiB pieces per workgroup and per wave (0: no pre-touch)
    uint32_t mul_hw, mul_wd, mul_pw;  // / (Hout * Wout), / Wout (halo: Hin * Win, Win), / (Win + 2) (halo patch)
    uint32_t geom;        // halo: Win | TH << 8 | PW << 16 | pit << 24
    uint32_t per_sc;      // halo: tail chunks per split
};
static_assert(sizeof(GemmHead) == 128, "the head is two 64-byte lines");

MRISR_GH_HD uint32_t gh_shift(const GemmHead& h, int field) { return (h.shifts >> field) & 31u; }

// what the host knows about a launch (GemmArgs restated without HIP types, plus the tile and what launch_gemm decided)
struct GemmHeadIn {
    const void *w = nullptr, *a0 = nullptr, *a1 = nullptr;
    int M = 0, N = 0, K = 0, c0 = 0, c1 = 0, lda0 = 0, lda1 = 0;
    int conv = 0, B = 0, Hin = 0, Win = 0, Hout = 0, Wout = 0, ups = 0, zstuff = 0, subpix = 0;
    int cs0 = 0, cs1 = 0, splitk = 1, batch = 1, group_m = 1, pretouch = 0, dbg = 0, stamped = 0;
    int BM = 64, BN = 64, halo = 0;
};

static inline uint32_t gh_clamp_extent(long long bytes) { return (uint32_t)(bytes < 0x7FFFFFFFll ? bytes : 0x7FFFFFFFll); }

inline GemmHead make_gemm_head(const GemmHeadIn& in) {
    GemmHead h{};
    h.w = in.w; h.a0 = in.a0; h.a1 = in.a1;
    const long long a_rows = in.conv ? (long long)in.B * in.Hin * in.Win : (long long)in.M;
    h.ext_w = gh_clamp_extent((long long)in.N * in.K * 2);
    h.ext_a0 = gh_clamp_extent(a_rows * in.lda0 * 2);
    h.ext_a1 = in.a1 ? gh_clamp_extent(a_rows * in.lda1 * 2) : 0u;
    h.flags = ((uint32_t)in.dbg & GH_DBG_MASK) | (in.conv ? GH_CONV : 0u) | (in.subpix ? GH_SUBPIX : 0u) | (in.zstuff ? GH_ZSTUFF : 0u) |
              (in.ups ? GH_UPS : 0u) | (in.a1 ? GH_A1 : 0u) | (in.cs0 ? GH_TAIL : 0u) | (in.stamped ? GH_STAMPED : 0u) |
              (in.batch > 1 ? GH_BATCHED : 0u);
    h.rows = (uint32_t)(in.halo ? in.Hin : in.M);
    h.N = (uint32_t)in.N;
    h.wpitch = (uint32_t)in.K * 2u;
    h.lda0 = (uint32_t)in.lda0; h.lda1 = (uint32_t)in.lda1; h.c0 = (uint32_t)in.c0;
    h.ntn = (uint32_t)((in.N + in.BN - 1) / in.BN);
    h.ntm = (uint32_t)(in.halo ? in.M / in.BM : (in.M + in.BM - 1) / in.BM);
    const uint32_t GM = (uint32_t)(in.group_m > 1 ? in.group_m : 1);
    h.group_m = GM;
    const uint32_t last = h.ntm % GM ? h.ntm % GM : GM;  // size of the last group (the only one that can be short)
    const MagicDiv pg = magic_for(GM * h.ntn), gm = magic_for(GM), ls = magic_for(last);
    h.mul_pg = pg.mul; h.mul_gm = gm.mul; h.mul_last = ls.mul;
    const int Ct = in.c0 + in.c1;
    h.Ct = (uint32_t)Ct;
    const int units = in.halo ? Ct / 64 : in.K / 64;
    h.per = (uint32_t)((units + in.splitk - 1) / in.splitk);
    h.per_sc = (uint32_t)(((in.cs0 + in.cs1) / 64 + in.splitk - 1) / in.splitk);
    if (in.pretouch > 0) {  // as pretouch_weights divided it: the shares of all workgroups cover the matrix once
        const long long pieces = ((long long)in.N * in.K * 2 + 1023) >> 10;
        const long long n_wg = (long long)h.ntn * h.ntm * in.splitk;
        const int per_wg = (int)((pieces + n_wg - 1) / n_wg);
        const int per_wave = (per_wg + 3) >> 2;
        h.pt_per_wg = (uint32_t)per_wg;
        h.pt_per_wave = (uint32_t)(per_wave < in.pretouch ? per_wave : in.pretouch);
    }
    MagicDiv hw = magic_for(1), wd = magic_for(1), pw = magic_for(1);
    if (in.halo) {
        const int TH = in.BM / in.Win, PW = in.Win + 2, npix = (TH + 2) * PW, pit = (npix * 8 + 255) / 256;
        hw = magic_for((uint32_t)(in.Hin * in.Win)); wd = magic_for((uint32_t)in.Win); pw = magic_for((uint32_t)PW);
        h.geom = (uint32_t)in.Win | (uint32_t)TH << 8 | (uint32_t)PW << 16 | (uint32_t)pit << 24;
    } else if (in.conv) {
        hw = magic_for((uint32_t)(in.Hout * in.Wout)); wd = magic_for((uint32_t)in.Wout);
    }
    h.mul_hw = hw.mul; h.mul_wd = wd.mul; h.mul_pw = pw.mul;
    h.shifts = pg.l << GH_SH_PG | gm.l << GH_SH_GM | ls.l << GH_SH_LAST | hw.l << GH_SH_HW | wd.l << GH_SH_WD | pw.l << GH_SH_PW;
    return h;
}

// ---- decoding (the kernels' own code: the checker calls exactly these) -----------------------------------------------------------
// workgroup blockIdx.x -> (tm, tn): the XCD remap (consecutive blockIdx.x go round the eight XCDs; each XCD takes a contiguous run of logical
// tiles), then the grouped order (within a group of group_m M tiles walk M first)
MRISR_GH_HD void gh_tile_coords(const GemmHead& h, uint32_t bid, uint32_t& tm, uint32_t& tn) {
    const uint32_t nblk = h.ntn * h.ntm;
    const uint32_t xcd = bid & 7u, q = nblk >> 3, r = nblk & 7u;
    const uint32_t logical = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (bid >> 3);
    const uint32_t per_group = h.group_m * h.ntn;
    const uint32_t grp = magic_div(logical, h.mul_pg, gh_shift(h, GH_SH_PG));
    const uint32_t first_m = grp * h.group_m;
    const uint32_t left = h.ntm - first_m;
    const bool full = h.group_m <= left;
    const uint32_t gsz = full ? h.group_m : left;
    const uint32_t within = logical - grp * per_group;
    tn = magic_div(within, full ? h.mul_gm : h.mul_last, gh_shift(h, full ? GH_SH_GM : GH_SH_LAST));
    tm = first_m + (within - tn * gsz);
}
// split blockIdx.y -> [beg, end) of `total` K tiles / chunks
MRISR_GH_HD void gh_split_range(uint32_t per, uint32_t total, uint32_t split, int& beg, int& end) {
    const uint32_t b = split * per, e = b + per;
    beg = (int)b;
    end = (int)(e < total ? e : total);
}
// conv row m -> (b, oy, ox) over a Hout x Wout map
MRISR_GH_HD void gh_row_pixel(const GemmHead& h, uint32_t m, uint32_t hw, uint32_t wout, uint32_t& b, uint32_t& oy, uint32_t& ox) {
    b = magic_div(m, h.mul_hw, gh_shift(h, GH_SH_HW));
    const uint32_t rem = m - b * hw;
    oy = magic_div(rem, h.mul_wd, gh_shift(h, GH_SH_WD));
    ox = rem - oy * wout;
}
MRISR_GH_HD uint32_t gh_div_pw(const GemmHead& h, uint32_t x) { return magic_div(x, h.mul_pw, gh_shift(h, GH_SH_PW)); }
MRISR_GH_HD uint32_t gh_div_wd(const GemmHead& h, uint32_t x) { return magic_div(x, h.mul_wd, gh_shift(h, GH_SH_WD)); }

}  // namespace mrisr
