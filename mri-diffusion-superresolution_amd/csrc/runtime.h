// Host-side runtime pieces shared by model.hip / capi.hip / sampler.hip / adapter.hip: device buffers, the bump arena, packed weights.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mrisr.h"
#include "common.h"

namespace mrisr {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int reserve(size_t n, bool zero) {
        if (n <= bytes) return 0;
        release();
        MRISR_CHECK_HIP(hipMalloc(&p, n));
        bytes = n;
        if (zero) MRISR_CHECK_HIP(hipMemset(p, 0, n));
        return 0;
    }
};

// "No buffer yet": a non-null address that is never dereferenced.  The dry pass of the arena hands out offsets from it, and a GEMM that is
// planned before its buffers are allocated carries kUnallocated in their place: gemm_choose decides from the signature of a launch, and
// WHICH operands exist (a residual, an output) is part of that signature.
constexpr uintptr_t kUnallocatedAddr = 0x1000;
static void* const kUnallocated = reinterpret_cast<void*>(kUnallocatedAddr);

// Bump allocator with stack discipline.  In `dry` mode it only tracks the peak, so one dry pass of the
// forward sizes the workspace exactly and every later pass reproduces the same addresses (hipGraph-safe).
struct Arena {
    DevBuf buf;
    size_t off = 0, peak = 0;
    bool dry = false;
    void reset() { off = 0; }
    void* alloc(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        off = a + bytes;
        if (off > peak) peak = off;
        if (dry) return reinterpret_cast<void*>(kUnallocatedAddr + a);
        if (off > buf.bytes) return nullptr;
        return static_cast<char*>(buf.p) + a;
    }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
};

struct RawParam {
    std::shared_ptr<DevBuf> data;  // f32
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

struct NormW {
    const float* g = nullptr;
    const float* b = nullptr;
    int c = 0;
    std::string name;  // state-dict module name (full-parameter training writes its affine gradients by name)
};
struct ConvW {  // packed [cout][ks*ks*cin] in compute dtype, bias f32
    void* w = nullptr;
    const float* b = nullptr;
    int cin = 0, cout = 0, ks = 3;
    std::string name;    // state-dict module name (the dgrad packer re-reads the raw f32 weight)
    void* wd = nullptr;  // training: dgrad filter bank [cin][ky'][kx'][cout] (taps flipped; 1x1: W^T [cin][cout]), compute dtype
    long long offW = -1, offB = -1;  // training (T2I-Adapter): offsets of weight / bias in the flat trainable vector
    // LoRA (peft lora.Conv2d on a resnet's conv1 / conv2; lora_conv.hip): the rank and the device views of lora_A [r][cin][3][3] and
    // lora_B [cout][r][1][1], B already scaled by lora_alpha / r
    int r = 0;
    void* loraA = nullptr;    // [r][ky][kx][cin] compute dtype: the down-projection z = conv3x3(x, A)
    void* loraAd = nullptr;   // bf16 engine: the tap-flipped dgrad bank [cin][conv_lora_kpad(r)]
    float* loraB = nullptr;   // f32 [cout][r]: the conv's epilogue (GemmArgs::lora_b)
    void* loraBT = nullptr;   // [r][cout] compute dtype: dz = dY (s B) through launch_lora_down
    long long offLA = -1, offLB = -1;  // training: offsets of lora_A / lora_B in the flat trainable vector
};
struct LinW {  // packed [n][k] in compute dtype, bias f32 (GEGLU: interleaved)
    void* w = nullptr;
    const float* b = nullptr;
    int n = 0, k = 0;
    int geglu_half = 0;  // > 0 (= n / 2): rows stored in the GEGLU interleave; raw row g * half + j sits at (j >> 4) * 32 + (j & 15) + 16 g
    // fused LoRA (peft): per fused module one rank-r adapter.  loraA [R = nmod*r][k] compute dtype, loraB f32 [n][r]
    // already scaled by lora_alpha/r; output column n uses z columns (n / secN) * r .. +r.  loraB / loraBT follow the row order of w
    // (geglu_half: interleaved)
    int r = 0, R = 0, secN = 1;
    // rank 32 .. 128: rp = r rounded up to the K tile, R = nmod * rp; loraA is [R][k] with module j's rows at j * rp, and
    // w is [n][k + R]: W, then (alpha/r) B_j in columns k + j * rp on module j's rows.  No loraB / loraAT; wT is [k][n + R] = [W^T | A^T]
    int rp = 0;
    int kw() const { return rp ? k + R : k; }  // row pitch of w
    void* loraA = nullptr;
    const float* loraB = nullptr;
    // fp8 copies for the row-panel kernel (cfg.fp8_linears; K = 320 / 640 only): e4m3 rows + one f32 scale per row
    void* w8 = nullptr;
    float* w_scale = nullptr;
    void* loraA8 = nullptr;       // [16][k] (rows >= R zero)
    float* loraA_scale = nullptr; // [16]
    // training
    std::vector<std::string> mod_names;  // the fused modules, in column order (e.g. attn1.to_q, to_k, to_v)
    std::vector<int> mod_lora;           // 1 if that module carries an adapter
    std::vector<long long> offA, offB;   // offsets of lora_A / lora_B of each module in the flat trainable vector (-1: none)
    void* wT = nullptr;                  // [k][n] compute dtype (dgrad operand)
    void* loraBT = nullptr;              // [R][n] compute dtype: (alpha/r) * B^T, zero outside the module's columns
    float* loraAT = nullptr;             // [k][R] f32: A^T (epilogue operand of the dgrad)
    float* loraB_rw = nullptr;           // writable alias of loraB (refreshed from the trainable vector)
    // DoRA: g = m / ||W + s B A|| per row of w (f32 [n], row order of w); w rows and the B bank are stored scaled by it
    float* dora_g = nullptr;
    std::vector<long long> offM;         // offsets of the magnitudes of each module in the flat trainable vector (-1: none)
};

struct Act {  // NHWC activation (or token rows when H*W is the token count)
    void* p = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    size_t rows() const { return (size_t)B * H * W; }
    size_t numel() const { return rows() * C; }
};

inline int dtype_size(int dt) { return dt == MRISR_F32 ? 4 : (dt == MRISR_I64 ? 8 : 2); }

// ---- tiled sampling (tiles.hip) ----
// one axis of the grid: increasing origins and the normalised window table [n_tiles][min(t, n)] (float64, rounded once to f32)
int tile_axis(int n, int t, int o, int window, std::vector<int>& origins, std::vector<float>& weights);
// both axes on the host, and their image as ONE small device upload: [oy | ox | pad][nwy | pad][nwx], each part on a 16-byte boundary
struct TilePlan {
    int H = 0, W = 0, th = 0, tw = 0;
    std::vector<int> oy, ox;
    std::vector<float> nwy, nwx;
    std::vector<uint32_t> words;
    size_t off_nwy = 0, off_nwx = 0;
    int T() const { return (int)(oy.size() * ox.size()); }
    int build(int H_, int W_, int tile_h, int tile_w, int overlap_h, int overlap_w, int window);  // the grid rule and the window
    int check();  // origins in range, increasing and covering; table sizes (explicit arrays of the single-op entries)
    void pack();
    size_t bytes() const { return words.size() * sizeof(uint32_t); }
    TileGrid grid(const void* dev) const;  // dev: where `words` was uploaded
};

}  // namespace mrisr
