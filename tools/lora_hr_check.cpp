// Stand-alone host check of the high-rank LoRA index arithmetic (csrc/lora_hr.h): walks the rank / module-count / width / row-count grid and
// replays every address the lora_wgrad_hr kernels form - the staged loads of P and Q, the partial tiles, the scatter into the gradient
// tensors - against buffers of exactly the advertised sizes.  Build it with the host sanitizers and run it on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I mri-diffusion-superresolution_amd/csrc \
//       tools/lora_hr_check.cpp -o build/lora_hr_check && build/lora_hr_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lora_hr.h"

using namespace mrisr;

static long long g_checked = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::abort();                                                             \
        }                                                                             \
        ++g_checked;                                                                  \
    } while (0)

static int geglu_raw_row(int packed, int half) { return ((packed >> 4) & 1) * half + (packed >> 5) * 16 + (packed & 15); }

// one launch of lora_wgrad_hr (bf16) on the host: every index touches a real byte, so the sanitizer sees an overrun
static void replay(int M, int C, int mode, int r, int nmod, int secN, int ldp, int ldq, int half) {
    const int rp = lora_hr_rp(r, 2);
    const LoraHrGeom g = lora_wgrad_hr_geom(M, C, mode, rp, nmod, secN);
    CHECK(g.rows % HR_STEP == 0 && g.gz >= 1 && g.gz <= HR_MAX_SLABS && (long long)g.gz * g.rows >= M && (long long)(g.gz - 1) * g.rows < M);
    std::vector<unsigned char> P((size_t)M * ldp, 0), Q((size_t)M * ldq, 0);  // touched flags, one per element
    std::vector<unsigned char> partial(lora_wgrad_hr_partial_floats(g), 0);
    std::vector<std::vector<unsigned char>> out(nmod);
    for (int j = 0; j < nmod; ++j) out[j].assign((size_t)(mode == 0 ? secN : C) * r, 0);
    std::vector<unsigned char> chan(C, 0);
    for (int tile = 0; tile < g.tiles; ++tile)
        for (int qb = 0; qb < g.qblk; ++qb) {
            int c0, cend, qcol0;
            lora_wgrad_hr_tile(g, mode, C, rp, secN, tile, qb, c0, cend, qcol0);
            CHECK(c0 % 8 == 0 && c0 < cend && cend <= C && (cend - c0) % 8 == 0 && qcol0 % HR_TQ == 0 && qcol0 + HR_TQ <= nmod * rp && qcol0 / rp < nmod);
            for (int z = 0; z < g.gz; ++z) {
                const int m_beg = z * g.rows, m_end = m_beg + g.rows < M ? m_beg + g.rows : M;
                CHECK(m_beg < m_end);
                const int nsteps = (m_end - m_beg + HR_STEP - 1) / HR_STEP;
                for (int step = 0; step < nsteps; step += (nsteps > 2 ? nsteps - 1 : 1))  // first and last step: the ragged one is the last
                    for (int t = 0; t < 256; ++t) {
                        const int m = m_beg + step * HR_STEP + (t >> 3), sch = (t & 7) * 8;
                        if (m >= m_end) continue;
                        if (c0 + sch < cend)
                            for (int e = 0; e < 8; ++e) P[(size_t)m * ldp + c0 + sch + e] = 1;
                        for (int e = 0; e < 8; ++e) Q[(size_t)m * ldq + qcol0 + sch + e] = 1;
                    }
                const size_t base = (((size_t)z * g.tiles + tile) * g.qblk + qb) * (HR_TC * HR_TQ);
                partial[base] = 1;
                partial[base + HR_TC * HR_TQ - 1] = 1;
            }
            for (int cl = 0; cl < HR_TC; ++cl)
                for (int ql = 0; ql < HR_TQ; ++ql) {
                    const int c = c0 + cl, qq = qcol0 + ql, j = qq / rp, q = qq - j * rp;
                    if (c >= cend || q >= r) continue;
                    if (qb == 0 && ql == 0) { CHECK(!chan[c]); chan[c] = 1; }
                    size_t at;
                    if (half) at = (size_t)geglu_raw_row(c, half) * r + q;
                    else if (mode == 0) at = (size_t)(c - j * secN) * r + q;
                    else at = (size_t)q * C + c;
                    CHECK(!out[j][at]);  // every gradient element exactly once
                    out[j][at] = 1;
                }
        }
    for (int c = 0; c < C; ++c) CHECK(chan[c]);
    for (int j = 0; j < nmod; ++j)
        for (unsigned char v : out[j]) CHECK(v);
}

int main() {
    for (int es : {2, 4})
        for (int r = 32; r <= 128; r += 16) {
            const int kt = lora_hr_ktile(es), rp = lora_hr_rp(r, es);
            CHECK(lora_rank_high(r) && !lora_rank_low(r) && rp % kt == 0 && rp >= r && rp - r < kt);
            for (int nmod = 1; nmod <= 3; ++nmod) {
                CHECK(lora_hr_Rp(r, nmod, es) == nmod * rp);
                for (int k : {64, 320, 1280})
                    for (int j = 0; j < nmod; ++j) CHECK(lora_hr_wcol(k, j, rp) + rp <= k + lora_hr_Rp(r, nmod, es) && lora_hr_wcol(k, j, rp) % kt == 0);
            }
        }
    for (int r : {0, 2, 6, 20, 24, 40, 144, 256}) CHECK(!lora_rank_high(r) && !lora_rank_low(r));
    for (int r : {4, 8, 12, 16}) CHECK(lora_rank_low(r) && !lora_rank_high(r));
    for (int r : {32, 48, 64, 128})
        for (int nmod : {1, 2, 3})
            for (int W : {8, 64, 104, 320, 1280})
                for (int M : {1, 31, 154, 1024, 4136, 65536 + 8}) {
                    if (M > 5000 && (W > 320 || r > 32)) continue;
                    const int rp = lora_hr_rp(r, 2);
                    replay(M, nmod * W, 0, r, nmod, W, nmod * W + 16, nmod * rp, 0);   // dB, P with a wider pitch
                    replay(M, W, 1, r, nmod, 320, W, nmod * rp + 40, 0);             // dA, Q with a wider pitch
                }
    for (int half : {16, 160, 1280}) replay(154, 2 * half, 0, 32, 1, 2 * half, 2 * half, 64, half);  // the GEGLU scatter
    std::printf("lora_hr_check: %lld checks passed\n", g_checked);
    return 0;
}
