// Stand-alone host check of the launch head of the tiled and halo GEMM kernels (csrc/gemm_head.h).  For a list of launches - every
// tiled / halo signature of the shipped tile table (profiles/r03_tune_cache.tsv, given as the argument) and the shapes of
// tests/test_gpu_gemm_head.py - it fills the head as the launchers do and compares what the kernels decode from it (the header's own inline
// functions: the kernels call the same ones) with the plain `/` and `%` the kernels used before the head existed: (tm, tn) of every
// blockIdx.x, the split range of every blockIdx.y, (b, oy, ox) of every conv row, the halo tile's image and first row, (hy, hx) of every patch
// transfer of every lane, prow of every fragment row, the pre-touch shares and the descriptor extents.  Every multiplier it meets is also held
// against true division: the sufficient condition 2^(31+l) <= mul * d <= 2^(31+l) + 2^l (which covers every dividend below 2^31), all dividends
// below 2^18 one by one, and both sides of every multiple of d (or of 2^16 evenly spaced ones) up to 2^31 - 1.  Any mismatch aborts.  Build with the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mri-diffusion-superresolution_amd/csrc
//       tools/gemm_head_check.cpp -o build/gemm_head_check && build/gemm_head_check profiles/r03_tune_cache.tsv      (one command line)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "gemm_head.h"

using namespace mrisr;

static long long g_checked = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: check failed: %s   [%s]\n", __FILE__, __LINE__, #cond, g_what.c_str()); \
            std::abort();                                                                 \
        }                                                                                 \
        ++g_checked;                                                                      \
    } while (0)
static std::string g_what;

// the tiled and halo lines of the tile registry (csrc/gemm.hip: TILES): id, BM, BN, halo
struct TileDim { int id, BM, BN, halo; };
static const TileDim kTiles[] = {
    {14, 128, 128, 0}, {15, 256, 64, 0}, {16, 128, 64, 0}, {17, 64, 64, 0}, {18, 64, 128, 0}, {25, 128, 160, 0}, {26, 64, 160, 0}, {27, 160, 160, 0},
    {28, 128, 192, 0}, {29, 192, 128, 0}, {30, 160, 128, 0}, {31, 96, 160, 0}, {32, 64, 64, 0}, {33, 64, 64, 0}, {34, 64, 128, 0}, {35, 128, 64, 0},
    {36, 128, 128, 0}, {37, 128, 160, 0}, {38, 128, 128, 0}, {39, 64, 160, 0}, {41, 128, 160, 1}, {42, 128, 128, 1}, {43, 64, 160, 1}, {44, 128, 192, 1},
    {45, 256, 64, 1},
};
static const TileDim* tile_dim(int id) {
    for (const TileDim& t : kTiles)
        if (t.id == id) return &t;
    return nullptr;
}

// ---- the multipliers against true division ----
static std::set<uint32_t> g_divisors_done;
static void check_divisor(uint32_t d) {
    if (!g_divisors_done.insert(d).second) return;
    const MagicDiv m = magic_for(d);
    CHECK(m.l <= 31);
    const unsigned __int128 md = (unsigned __int128)m.mul * d, p = (unsigned __int128)1 << (31 + m.l);
    CHECK(md >= p && md <= p + ((unsigned __int128)1 << m.l));
    for (uint32_t x = 0; x < (1u << 18); ++x) CHECK(magic_div(x, m.mul, m.l) == x / d);
    const uint64_t top = 0x7FFFFFFFull, nmul = top / d;
    const uint64_t step = nmul > (1ull << 16) ? nmul >> 16 : 1;
    for (uint64_t k = 1; k <= nmul; k += step) {
        const uint32_t x = (uint32_t)(k * d);
        CHECK(magic_div(x, m.mul, m.l) == x / d);
        CHECK(magic_div(x - 1, m.mul, m.l) == (x - 1) / d);
    }
    const uint32_t xl = (uint32_t)(nmul * d);
    CHECK(magic_div(xl, m.mul, m.l) == xl / d && magic_div(xl - 1, m.mul, m.l) == (xl - 1) / d);
    CHECK(magic_div((uint32_t)top, m.mul, m.l) == (uint32_t)top / d);
}

// ---- one launch ----
static void check_launch(const GemmHeadIn& in, const char* what) {
    g_what = what;
    const GemmHead h = make_gemm_head(in);
    const int BM = in.BM, BN = in.BN;
    // extents, as the kernels clamped them
    const long long a_rows = in.conv ? (long long)in.B * in.Hin * in.Win : (long long)in.M;
    CHECK(h.ext_w == (unsigned)std::min((long long)in.N * in.K * 2, 0x7FFFFFFFll));
    CHECK(h.ext_a0 == (unsigned)std::min(a_rows * in.lda0 * 2, 0x7FFFFFFFll));
    CHECK(h.ext_a1 == (in.a1 ? (unsigned)std::min(a_rows * in.lda1 * 2, 0x7FFFFFFFll) : 0u));
    // (tm, tn) for every blockIdx.x
    const int ntn = (in.N + BN - 1) / BN, ntm = in.halo ? in.M / BM : (in.M + BM - 1) / BM, nblk = ntn * ntm;
    CHECK((int)h.ntn == ntn && (int)h.ntm == ntm);
    std::vector<char> seen((size_t)nblk, 0);
    for (int bid = 0; bid < nblk; ++bid) {
        int logical;
        {
            const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
            logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
        }
        const int GM = in.group_m > 1 ? in.group_m : 1;
        const int per_group = GM * ntn;
        const int grp = logical / per_group;
        const int first_m = grp * GM;
        const int gsz = std::min(GM, ntm - first_m);
        const int within = logical - grp * per_group;
        const int tm = first_m + within % gsz, tn = within / gsz;
        uint32_t tm_h, tn_h;
        gh_tile_coords(h, (uint32_t)bid, tm_h, tn_h);
        CHECK((int)tm_h == tm && (int)tn_h == tn);
        CHECK(tm >= 0 && tm < ntm && tn >= 0 && tn < ntn && !seen[(size_t)tm * ntn + tn]);  // (and the order is a permutation of the tiles)
        seen[(size_t)tm * ntn + tn] = 1;
    }
    check_divisor((uint32_t)((in.group_m > 1 ? in.group_m : 1) * ntn));
    check_divisor((uint32_t)(in.group_m > 1 ? in.group_m : 1));
    // split ranges for every blockIdx.y
    const int Ct = in.c0 + in.c1;
    const int units = in.halo ? Ct / 64 : in.K / 64;
    CHECK(in.halo ? (int)h.Ct / 64 == units : (int)(h.wpitch >> 7) == units);
    const int nsc = (in.cs0 + in.cs1) / 64;
    if (in.halo) CHECK((int)(h.wpitch >> 7) - 9 * units == nsc);
    for (int split = 0; split < in.splitk; ++split) {
        const int per = (units + in.splitk - 1) / in.splitk;
        const int beg = split * per, end = std::min(units, beg + per);
        int b, e;
        gh_split_range(h.per, (uint32_t)units, (uint32_t)split, b, e);
        CHECK(b == beg && e == end);
        if (in.halo) {
            const int per_sc = (nsc + in.splitk - 1) / in.splitk;
            const int sc_beg = std::min(nsc, split * per_sc), sc_end = std::min(nsc, sc_beg + per_sc);
            const int sb = std::min(nsc, split * (int)h.per_sc), se = std::min(nsc, sb + (int)h.per_sc);
            CHECK(sb == sc_beg && se == sc_end);
        }
    }
    // pre-touch shares
    if (in.pretouch > 0) {
        const long long w_bytes = (long long)in.N * in.K * 2;
        const int n_wg = nblk * in.splitk;
        const long long pieces = (w_bytes + 1023) >> 10;
        const int per_wg = (int)((pieces + n_wg - 1) / n_wg);
        const int per_wave = std::min((per_wg + 3) >> 2, in.pretouch);
        CHECK((int)h.pt_per_wg == per_wg && (int)h.pt_per_wave == per_wave && (long long)((h.ext_w + 1023u) >> 10) == pieces);
        for (int wg = 0; wg < n_wg; ++wg)
            for (int wave = 0; wave < 4; ++wave) {
                const long long first = (long long)wg * per_wg + (long long)wave * per_wave;
                CHECK((long long)((unsigned)wg * h.pt_per_wg + (unsigned)wave * h.pt_per_wave) == first);
            }
    } else {
        CHECK(h.pt_per_wave == 0);
    }
    if (in.halo) {
        const int Wd = in.Win, Hd = in.Hin, TH = BM / Wd, PW = Wd + 2, npix = (TH + 2) * PW, pit = (npix * 8 + 255) / 256;
        CHECK((int)(h.geom & 255u) == Wd && (int)(h.geom >> 8 & 255u) == TH && (int)(h.geom >> 16 & 255u) == PW && (int)(h.geom >> 24) == pit && (int)h.rows == Hd);
        for (int tm = 0; tm < ntm; ++tm) {  // the tile's image and first row
            const int m0 = tm * BM;
            const int img = m0 / (Hd * Wd), y0 = (m0 - img * Hd * Wd) / Wd;
            const int img_h = (int)magic_div((uint32_t)m0, h.mul_hw, gh_shift(h, GH_SH_HW));
            CHECK(img_h == img && (int)gh_div_wd(h, (uint32_t)(m0 - img_h * Hd * Wd)) == y0);
        }
        const int PIT_MAX = BM >= 256 ? 13 : (BM >= 128 ? 9 : 6);
        CHECK(pit <= PIT_MAX);
        for (int it = 0; it < PIT_MAX; ++it)  // every transfer of every lane
            for (int tid = 0; tid < 256; ++tid) {
                const int pp = (it * 256 + tid) >> 3;
                const int hy = pp / PW, hx = pp - hy * PW;
                const int hy_h = (int)gh_div_pw(h, (uint32_t)pp);
                CHECK(hy_h == hy && pp - hy_h * PW == hx);
            }
        for (int p = 0; p < BM; ++p) {  // prow of every row of the tile
            const int ty = p / Wd, tx = p - ty * Wd;
            const int ty_h = (int)gh_div_wd(h, (uint32_t)p);
            CHECK(ty_h == ty && ty_h * PW + (p - ty_h * Wd) == ty * PW + tx);
        }
        check_divisor((uint32_t)(Hd * Wd)); check_divisor((uint32_t)Wd); check_divisor((uint32_t)PW);
    } else if (in.conv) {
        CHECK((int)h.rows == in.M);
        const int hw = in.Hout * in.Wout;
        for (int m = 0; m < in.M; ++m) {  // (b, oy, ox) of every row
            const int b = m / hw, rem = m - b * hw, oy = rem / in.Wout, ox = rem - oy * in.Wout;
            uint32_t bh, oyh, oxh;
            gh_row_pixel(h, (uint32_t)m, (uint32_t)hw, (uint32_t)in.Wout, bh, oyh, oxh);
            CHECK((int)bh == b && (int)oyh == oy && (int)oxh == ox);
        }
        check_divisor((uint32_t)hw); check_divisor((uint32_t)in.Wout);
    } else {
        CHECK((int)h.rows == in.M);
    }
    // flags
    CHECK(((h.flags & GH_CONV) != 0) == (in.conv != 0) && ((h.flags & GH_SUBPIX) != 0) == (in.subpix != 0) && ((h.flags & GH_ZSTUFF) != 0) == (in.zstuff != 0));
    CHECK(((h.flags & GH_UPS) != 0) == (in.ups != 0) && ((h.flags & GH_A1) != 0) == (in.a1 != nullptr) && ((h.flags & GH_TAIL) != 0) == (in.cs0 != 0));
    CHECK(((h.flags & GH_BATCHED) != 0) == (in.batch > 1) && (h.flags & GH_DBG_MASK) == ((uint32_t)in.dbg & 0xFFFFu));
}

static char g_dummy[8];
static int g_launches = 0;
static void run(GemmHeadIn in, int tile, const char* tag) {
    const TileDim* t = tile_dim(tile);
    if (!t) return;  // (a row-panel / weight-stationary line of the table: not these kernels)
    in.BM = t->BM; in.BN = t->BN; in.halo = t->halo;
    in.w = g_dummy; in.a0 = g_dummy; in.a1 = in.c1 ? g_dummy : nullptr;
    if (!in.lda0) in.lda0 = in.c0;
    if (!in.lda1) in.lda1 = in.c1;
    const int ntm = in.halo ? in.M / in.BM : (in.M + in.BM - 1) / in.BM;
    if (in.group_m == 0) in.group_m = std::max(1, std::min(8, ntm));  // auto_group_m
    if (in.pretouch < 0) in.pretouch = (in.batch == 1 && (long long)in.N * in.K * 2 >= 512 * 1024) ? 32 : 0;
    if (in.halo) {  // halo_geometry_ok
        if (!(in.conv && in.Win % 8 == 0 && in.Win <= 64 && in.BM % in.Win == 0 && (in.Hin * in.Win) % in.BM == 0 && in.M % in.BM == 0)) {
            std::fprintf(stderr, "%s on tile %d: not a geometry the halo kernels admit\n", tag, tile);
            std::abort();
        }
    }
    char what[256];
    std::snprintf(what, sizeof(what), "%s tile %d M=%d N=%d K=%d split=%d group_m=%d", tag, tile, in.M, in.N, in.K, in.splitk, in.group_m);
    check_launch(in, what);
    ++g_launches;
}

static GemmHeadIn plain(int M, int N, int K, int c1 = 0) {
    GemmHeadIn in;
    in.M = M; in.N = N; in.K = K; in.c0 = K - c1; in.c1 = c1; in.group_m = 0; in.pretouch = -1;
    return in;
}
static GemmHeadIn conv(int B, int H, int W, int Cin, int Cout, int stride, int ups, int pad, int kw = 3, int c1 = 0, int cs0 = 0, int cs1 = 0) {
    GemmHeadIn in;
    in.conv = 1; in.B = B; in.Hin = H; in.Win = W; in.ups = ups;
    in.Hout = pad ? ((H << ups) - 1) / stride + 1 : H / 2;
    in.Wout = pad ? ((W << ups) - 1) / stride + 1 : W / 2;
    in.M = B * in.Hout * in.Wout; in.N = Cout; in.c0 = Cin - c1; in.c1 = c1; in.cs0 = cs0; in.cs1 = cs1;
    in.K = kw * kw * Cin + cs0 + cs1; in.group_m = 0; in.pretouch = -1;
    return in;
}

// "M,N,K,cC,sS,uU,c0,c1,aA,oO,bB,rR,vV,hH,wW[,qQ][,tCS0,CS1]<TAB>tile<TAB>split"
static void run_table(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::abort(); }
    char line[512];
    int rows = 0;
    while (std::fgets(line, sizeof(line), f)) {
        int M, N, K, c, s, u, c0, c1, a, o, b, r, v, hh, ww, n = 0;
        if (std::sscanf(line, "%d,%d,%d,c%d,s%d,u%d,%d,%d,a%d,o%d,b%d,r%d,v%d,h%d,w%d%n", &M, &N, &K, &c, &s, &u, &c0, &c1, &a, &o, &b, &r, &v, &hh, &ww, &n) != 15) continue;
        int q = 0, cs0 = 0, cs1 = 0, tile = 0, split = 1;
        const char* p = line + n;
        if (std::sscanf(p, ",q%d%n", &q, &n) == 1) p += n;
        if (std::sscanf(p, ",t%d,%d%n", &cs0, &cs1, &n) == 2) p += n;
        if (std::sscanf(p, "%d %d", &tile, &split) != 2) continue;
        GemmHeadIn in;
        if (c) {
            const int pad = s >= 8 ? 0 : 1, stride = s >= 8 ? s - 8 : s, kw = q ? q / 2 : 3;
            const int Hout = q ? hh : (pad ? ((hh << u) - 1) / stride + 1 : hh / 2), Wout = q ? ww : (pad ? ((ww << u) - 1) / stride + 1 : ww / 2);
            in = conv(M / (Hout * Wout), hh, ww, c0 + c1, N, stride, u, pad, kw, c1, cs0, cs1);
            in.Hout = Hout; in.Wout = Wout; in.M = M; in.subpix = q & 1;
            if (in.K != K) { std::fprintf(stderr, "table row %s: K does not match its form\n", line); std::abort(); }
        } else {
            in = plain(M, N, K, c1);
        }
        in.batch = b; in.splitk = split;
        run(in, tile, "table");
        ++rows;
    }
    std::fclose(f);
    std::printf("  %d table rows read\n", rows);
}

int main(int argc, char** argv) {
    if (argc > 1) run_table(argv[1]);
    // ---- the shapes of tests/test_gpu_gemm_head.py ----
    for (int tile : {17, 26, 14, 25})
        for (int N : {68, 160, 192})
            for (int K : {128, 192}) {
                GemmHeadIn in = plain(272, N, K);
                in.lda0 = K + 8;
                run(in, tile, "plain");
                for (int gm : {1, 2, 3, 8}) { in.group_m = gm; run(in, tile, "plain group_m"); }
                if (K == 192) { in.group_m = 0; in.splitk = 2; run(in, tile, "plain split 2"); }
            }
    for (int tile : {17, 26, 14, 25}) {
        run(plain(8, 160, 128), tile, "one tile, 8 rows");
        run(plain(272, 160, 192, 128), tile, "two sources");
        GemmHeadIn bt = plain(272, 64, 128);
        bt.batch = 3;
        run(bt, tile, "batched");
        // tiled conv: B = 3 on a 6 x 10 map, C = 64 -> 64
        run(conv(3, 6, 10, 64, 64, 1, 0, 1), tile, "conv stride 1");
        run(conv(3, 6, 10, 64, 64, 2, 0, 0), tile, "conv stride 2 pad 0");
        run(conv(3, 6, 10, 64, 64, 1, 1, 1), tile, "conv nearest x2");
        GemmHeadIn zs = conv(3, 6, 10, 64, 64, 1, 1, 1);
        zs.zstuff = 1;
        run(zs, tile, "conv zero-stuffed x2");
        GemmHeadIn sp = conv(3, 6, 10, 64, 64, 1, 0, 1, 2);
        sp.subpix = 1; sp.batch = 4;
        run(sp, tile, "conv sub-pixel");
        run(conv(3, 6, 10, 64, 64, 1, 0, 1, 3, 0, 64, 0), tile, "conv + 1x1 tail");
        run(conv(3, 6, 10, 64, 64, 1, 0, 1, 3, 0, 64, 64), tile, "conv + 1x1 tail, two sources");
        run(conv(3, 6, 10, 128, 64, 1, 0, 1, 3, 64), tile, "conv two sources");
        GemmHeadIn cs = conv(3, 6, 10, 64, 64, 1, 0, 1);
        cs.splitk = 2;
        run(cs, tile, "conv split 2");
    }
    for (int tile : {41, 43})
        for (int hw : {8, 16, 32}) {
            const TileDim* t = tile_dim(tile);
            if (t->BM % hw || (hw * hw) % t->BM) continue;  // whole tiles per image
            run(conv(2, hw, hw, 64, 160, 1, 0, 1), tile, "halo");
            run(conv(2, hw, hw, 128, 160, 1, 0, 1, 3, 64), tile, "halo two sources");
            run(conv(2, hw, hw, 64, 160, 1, 0, 1, 3, 0, 64, 0), tile, "halo + 1x1 tail");
            GemmHeadIn s2 = conv(2, hw, hw, 128, 160, 1, 0, 1, 3, 0, 64, 64);
            s2.splitk = 2;
            run(s2, tile, "halo split 2 + tail");
            for (int gm : {1, 2, 3, 8}) { GemmHeadIn g = conv(2, hw, hw, 64, 160, 1, 0, 1); g.group_m = gm; run(g, tile, "halo group_m"); }
        }
    run(plain(272, 640, 448), 26, "plain, pre-touched weights");
    run(conv(2, 16, 16, 192, 160, 1, 0, 1), 41, "halo, pre-touched weights");
    // ---- the multipliers on their own: small divisors one by one, then powers of two and their neighbours up to 2^31 - 1 ----
    g_what = "divisors";
    for (uint32_t d = 1; d <= 300; ++d) check_divisor(d);
    for (int k = 9; k <= 30; ++k)
        for (int e = -1; e <= 1; ++e) check_divisor((1u << k) + (uint32_t)e);
    check_divisor(0x7FFFFFFFu);
    std::printf("gemm_head_check: %d launches, %zu divisors, %lld checks passed (GemmHead is %zu bytes)\n", g_launches, g_divisors_done.size(), g_checked, sizeof(GemmHead));
    return 0;
}
