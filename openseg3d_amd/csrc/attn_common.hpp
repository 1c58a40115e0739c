// Shared pieces of the window-attention kernels (attention.hip, attention_small.hip, attention_fused.hip,
// attention_fused_bwd.hip).  The split-bf16 arithmetic they run on is split_bf16.hpp's, re-exported into this namespace.
#pragma once
#include "split_bf16.hpp"

namespace attn {

using namespace sbf;

constexpr float kNormEps = 1e-12f;  // F.normalize eps, cosine_msa.py:152-153
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

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
