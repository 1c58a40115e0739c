// Shared pieces of the window-attention kernels (attention.hip, attention_small.hip, attention_fused.hip,
// attention_fused_bwd.hip).  The split-bf16 arithmetic they run on is split_bf16.hpp's, re-exported into this namespace.
#pragma once
#include "split_bf16.hpp"

#include "attn_dropout.hpp"  // after the HIP runtime's header: DropoutParams

// One window-attention call by name: what an entry of attention.hip hands to a launcher and the launcher hands on to
// launch<DH> / run_small_bwd, which unpack it only at the hipLaunchKernelGGL line.  Strides in floats, n_chunks <= n_tiles.
struct AttnArgs {
    const float *q, *k, *v;                      // operands: rows of heads x dh floats
    int ldq, ldk, ldv;
    const int32_t *tok, *win_start, *win_count;  // the window index (seg3d_window_partition)
    const int4* tile_item;                       // (window, 32-token tile) items, as the kernels read them
    int n_tiles;
    const int4* chunk_item;                      // (window, 128-token chunk) items: the header's qg_item
    int n_chunks;
    int64_t m;
    int heads, dh;
    const float* tau;                            // 1 (kShared) / heads (kPerHead) values, null in kDot
    float tau_min;
    int am;                                      // attn::kShared / kPerHead / kDot (below)
    DropoutParams drop;
    hipStream_t st;
};

struct AttnBwdArgs : AttnArgs {
    const float *out, *dout, *lse;
    float *dq, *dk, *dv;
    int lddq, lddk, lddv;
    float* dtau;      // 1 / heads values, written; null in kDot
    void* workspace;  // attn_fused_bwd_workspace_bytes / attn_small_blocks x (tau values) floats
};

// The launchers and queries behind the entry points of attention.hip, declared once for the file that defines them and
// for their callers.  Workspace sizes in bytes, block counts in workgroups.
// attention_fused.hip
bool attn_fused_supported(int heads, int dh);
int attn_fused_fwd_launch(const AttnArgs& a, float* out, float* lse);
int attn_fused_fwd_schedule(int n_tiles, int n_chunks, int heads, int dh, bool dropout, int* cap, int* grid, int* walked,
                            int* xb);
// attention_fused_bwd.hip
bool attn_fused_bwd_supported(int heads, int dh);
size_t attn_fused_bwd_blocks(int n_tiles, int n_chunks, int heads, int dh);
size_t attn_fused_bwd_workspace_bytes(int64_t m, int n_tiles, int n_chunks, int heads, int dh);
int attn_fused_bwd_launch(const AttnBwdArgs& a);
// attention_small.hip
bool attn_small_supported(int heads, int dh);
size_t attn_small_blocks(int n_tiles);
int attn_small_fwd_launch(const AttnArgs& a, float* out, float* lse);
int attn_small_bwd_launch(const AttnBwdArgs& a);

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

// f(std::integral_constant<int, AM>{}) for the run-time mode am: where a launcher's mode becomes a template argument.
// (The compiler emits a file's kernels in the order their instantiations are first named: the cases keep the order the
// launchers always had, so that the device assembly still compares equal line by line -- tools/isa_diff.py.)
template <class F>
int for_attn_mode(int am, F&& f) {
    switch (am) {
        case kPerHead: return f(std::integral_constant<int, kPerHead>{});
        case kDot: return f(std::integral_constant<int, kDot>{});
        case kShared: return f(std::integral_constant<int, kShared>{});
        default: return SEG3D_EINVAL;
    }
}

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
