// Shared pieces of the window-attention kernels (attention.hip, attention_small.hip, attention_fused.hip,
// attention_fused_bwd.hip).  The split-bf16 arithmetic they run on is split_bf16.hpp's, re-exported into this namespace.
#pragma once
#include "split_bf16.hpp"

#include "attn_dropout.hpp"  // after the HIP runtime's header: DropoutParams

// The launchers and queries behind the entry points of attention.hip, declared once for the file that defines them and
// for their callers.  n_chunks <= n_tiles; workspace sizes in bytes, block counts in workgroups.
// attention_fused.hip
bool attn_fused_supported(int heads, int dh);
int attn_fused_fwd_launch(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const int32_t* tok,
                          const int32_t* win_start, const int32_t* win_count, const int32_t* tile_item, int n_tiles,
                          const int32_t* chunk_item, int n_chunks, int heads, int dh, const float* tau, float tau_min,
                          float* out, float* lse, float dropout_p, uint64_t seed, hipStream_t st, int am);
int attn_fused_fwd_schedule(int n_tiles, int n_chunks, int heads, int dh, bool dropout, int* cap, int* grid, int* walked,
                            int* xb);
// attention_fused_bwd.hip
bool attn_fused_bwd_supported(int heads, int dh);
size_t attn_fused_bwd_blocks(int n_tiles, int n_chunks, int heads, int dh);
size_t attn_fused_bwd_workspace_bytes(int64_t m, int n_tiles, int n_chunks, int heads, int dh);
int attn_fused_bwd_launch(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* out,
                          const float* dout, const float* lse, const int32_t* tok, const int32_t* win_start,
                          const int32_t* win_count, const int32_t* tile_item, int n_tiles, const int32_t* chunk_item,
                          int n_chunks, int64_t m, int heads, int dh, const float* tau, float tau_min, float* dq, float* dk,
                          float* dv, int lddq, int lddk, int lddv, float* dtau, void* workspace, const DropoutParams& drop,
                          hipStream_t st, int am);
// attention_small.hip
bool attn_small_supported(int heads, int dh);
size_t attn_small_blocks(int n_tiles);
int attn_small_fwd_launch(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const int32_t* tok,
                          const int32_t* win_start, const int32_t* win_count, const int32_t* tile_item, int n_tiles, int heads,
                          int dh, const float* tau, float tau_min, float* out, float* lse, const DropoutParams& drop,
                          hipStream_t st, int am);
int attn_small_bwd_launch(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* out,
                          const float* dout, const float* lse, const int32_t* tok, const int32_t* win_start,
                          const int32_t* win_count, const int32_t* tile_item, int n_tiles, int heads, int dh,
                          const float* tau, float tau_min, float* dq, float* dk, float* dv, int lddq, int lddk, int lddv,
                          float* dtau, void* workspace, const DropoutParams& drop, hipStream_t st, int am);

namespace attn {

using namespace sbf;

constexpr float kNormEps = 1e-12f;  // F.normalize eps, cosine_msa.py:152-153
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// Attention modes the kernels are instantiated for (the AM template argument; SEG3D_ATTN_COSINE / _DOT of the header):
//   kShared   cosine, one tau for all heads (cosine_msa.py:156-160 with non_shared_tau=False): the kernels as they were
//   kPerHead  cosine, tau[h] per head (non_shared_tau=True): every scale, bound and tau partial belongs to ONE head
//   kDot      scaled dot product (cosine_msa.py:163-165): no normalisation, scores q.k / sqrt(dh) are unbounded -- always
//             the running maximum, no tau
constexpr int kShared = 0, kPerHead = 1, kDot = 2;

// Masking streamed tokens past a window's end INSIDE the score product: the K dimension of the score MFMAs is padded from
// the stored head width DHS to a multiple of 32, so channel DHS is spare.  The stationary (query) fragment carries 1.0
// there, the streamed (key) fragment kMaskScore for a token past the end and 0 otherwise: the score of such a token comes
// out of the matrix core as -16384 + (a real row's score), exp2 of it is exactly 0 under any admissible temperature
// (scores are bounded by log2e / tau_min = 144), and no per-element compare / select is spent on it.
constexpr uint32_t kSpareOne = 0x3F80u;    // bf16 1.0 in element 0 of a fragment dword
constexpr uint32_t kSpareMask = 0xC680u;   // bf16 -16384.0

// slot of tile-local token r in the transposed arrays: token kappa(g, j) = (j < 4 ? 4g + j : 16 + 4g + j - 4)
// lives at slot 8g + j, so the 8 accumulator registers a lane holds after two 16-row MFMA tiles
// ([u=0: r 0..3, u=1: r 0..3]) are, in order, the k-slots of one 16-B transposed fragment.
__device__ __forceinline__ int perm_slot(int r) {
    return r < 16 ? (r >> 2) * 8 + (r & 3) : ((r - 16) >> 2) * 8 + 4 + ((r - 16) & 3);
}

template <int DH>
struct Geo {
    static constexpr int DHS = (DH + 7) / 8 * 8;  // stored channels per head (multiple of 8)
    static constexpr int KS = (DHS + 31) / 32;    // MFMA k-steps over the head dimension
    static constexpr int NB = (DH + 15) / 16;     // 16-row d-blocks of a transposed output
};

}  // namespace attn
