// Perturbed-attention guidance: identity attention.  With the softmax map of a self-attention block replaced by
// the identity, every token's attention output is its own value vector, so the block's attention output is V itself: no Q K^T, no
// softmax, no P V - only the way back from the head-major v^T the projection GEMM wrote to the token rows everything downstream reads.
//
//   vt [B*H][dpad][npad]  ->  out [B][N][H*hd]      for samples b0 <= b < b0 + nb; out[b][t][h*hd + d] = vt[b*H + h][d][t]
//
// A batched transpose of 2- or 4-byte elements, memory-bound: one workgroup moves a tile of ID_TD channels x ID_TN tokens of one
// (sample, head) through LDS, so that the global read runs along tokens and the global write along channels, both in 16-byte pieces.
// The tile lies in LDS in the source orientation, [channel][token], written with 16-byte stores; a 16-byte pad follows every VE channel
// rows (VE = elements per 16 bytes), so that the VE-channel groups one store-phase lane gathers from start 4 banks apart.  The gather is
// VE element-wise LDS reads per lane, one per channel; by the layout each of them is conflict-free within a 32-lane half: f32, 4 tokens
// x 8 groups read 32 distinct banks; bf16, 8 tokens x 4 groups read 16 banks (4 groups x 4 dwords), the two tokens of a dword sharing
// one address.  (Worked out from the bank rule, not measured with a conflict counter.)
// Pad columns (tokens >= N) may be read into LDS inside npad but are never stored; channels >= hd are never read.
#include "api.h"
#include "prof.h"
#include "runtime.h"

namespace mrisr {

constexpr int ID_TN = 64;  // tokens per tile
constexpr int ID_TD = 32;  // channels of one head per tile

template <typename T>
__device__ __forceinline__ int id_lds_at(int d, int tok) {
    constexpr int VE = 16 / (int)sizeof(T);
    return d * ID_TN + (d / VE) * VE + tok;
}

// vec_in: npad is a multiple of VE and vt is 16-byte aligned (every row piece is); vec_out: hd is a multiple of VE and out is aligned
template <typename T>
__global__ __launch_bounds__(256) void attn_identity_kernel(const T* __restrict__ vt, T* __restrict__ out, int H, int N, int hd, int npad,
                                                            int dpad, int b0, int tiles_n, int tiles_d, int vec_in, int vec_out) {
    constexpr int VE = 16 / (int)sizeof(T);
    __shared__ uint4 raw[(ID_TD * ID_TN + ID_TD) * sizeof(T) / 16];
    T* lds = reinterpret_cast<T*>(raw);
    int blk = blockIdx.x;
    const int tn = blk % tiles_n; blk /= tiles_n;
    const int td = blk % tiles_d; blk /= tiles_d;
    const int h = blk % H;
    const int b = b0 + blk / H;
    const int n0 = tn * ID_TN, d0 = td * ID_TD;
    const T* src = vt + ((size_t)b * H + h) * dpad * npad;
    // load: lanes run along tokens, one 16-byte piece each
    for (int v = threadIdx.x; v < ID_TD * (ID_TN / VE); v += 256) {
        const int tv = v % (ID_TN / VE), d = v / (ID_TN / VE);
        const int tok = n0 + tv * VE;
        if (d0 + d >= hd || tok >= N) continue;
        const T* p = src + (size_t)(d0 + d) * npad + tok;
        if (vec_in) {
            *reinterpret_cast<uint4*>(lds + id_lds_at<T>(d, tv * VE)) = *reinterpret_cast<const uint4*>(p);
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (tok + k < N) lds[id_lds_at<T>(d, tv * VE + k)] = p[k];
        }
    }
    __syncthreads();
    // store: lanes run along channels, one 16-byte piece (VE channels of one token) each
    const int C = H * hd;
    for (int v = threadIdx.x; v < ID_TN * (ID_TD / VE); v += 256) {
        const int dv = v % (ID_TD / VE), t = v / (ID_TD / VE);
        const int tok = n0 + t, d = d0 + dv * VE;
        if (tok >= N || d >= hd) continue;
        union { uint4 q; T e[VE]; } u;
#pragma unroll
        for (int k = 0; k < VE; ++k) u.e[k] = lds[id_lds_at<T>(dv * VE + k, t)];
        T* q = out + ((size_t)b * N + tok) * C + (size_t)h * hd + d;
        if (vec_out) {
            *reinterpret_cast<uint4*>(q) = u.q;
        } else {
#pragma unroll
            for (int k = 0; k < VE; ++k)
                if (d + k < hd) q[k] = u.e[k];
        }
    }
}

template <typename T>
int launch_attn_identity(const void* vt, void* out, int B, int H, int N, int hd, int npad, int dpad, int b0, int nb, hipStream_t st) {
    constexpr int VE = 16 / (int)sizeof(T);
    MRISR_REQUIRE(vt && out, "identity attention: null operand");
    MRISR_REQUIRE((reinterpret_cast<uintptr_t>(vt) % sizeof(T)) == 0 && (reinterpret_cast<uintptr_t>(out) % sizeof(T)) == 0,
                  "identity attention: misaligned operand");
    MRISR_REQUIRE(B > 0 && H > 0 && N > 0 && hd > 0, "identity attention: empty geometry");
    MRISR_REQUIRE(npad >= N, "identity attention: npad must be at least N");
    MRISR_REQUIRE(dpad >= hd, "identity attention: dpad must be at least hd");
    MRISR_REQUIRE(b0 >= 0 && nb >= 0 && (long long)b0 + nb <= B, "identity attention: the sample range lies outside B");
    if (nb == 0) return 0;
    const int tiles_n = (N + ID_TN - 1) / ID_TN, tiles_d = (hd + ID_TD - 1) / ID_TD;
    const long long blocks = (long long)tiles_n * tiles_d * H * nb;
    MRISR_REQUIRE(blocks < (1ll << 31), "identity attention: too many tiles for one launch");
    const int vec_in = npad % VE == 0 && reinterpret_cast<uintptr_t>(vt) % 16 == 0;
    const int vec_out = hd % VE == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    ProfScope ps("attn_identity", 0.0, 2.0 * nb * H * (double)N * hd * sizeof(T), st);
    hipLaunchKernelGGL(attn_identity_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const T*>(vt), static_cast<T*>(out), H, N,
                       hd, npad, dpad, b0, tiles_n, tiles_d, vec_in, vec_out);
    MRISR_CHECK_HIP(hipGetLastError());
    return 0;
}
template int launch_attn_identity<float>(const void*, void*, int, int, int, int, int, int, int, int, hipStream_t);
template int launch_attn_identity<bf16>(const void*, void*, int, int, int, int, int, int, int, int, hipStream_t);

}  // namespace mrisr
