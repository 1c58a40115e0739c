// Device code of the training criterion shared by its three translation units: the per-term entries (loss.hip: 'ce' /
// 'ohem_ce', lovasz.hip: 'lovasz') and the fused entry over all heads and both terms (criterion.hip).  Every quantity has
// ONE expression here, so that with -ffp-contract=off the fused entry returns the bits of the per-term ones.  The sums over
// a workgroup are wave_ops.hpp's (block_sum: wave xor tree, then the waves in ascending order), as in the other loss files.
#pragma once
#include "wave_ops.hpp"

namespace crit {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;           // row-pass workgroups per head (grid-stride beyond)
constexpr int kItems = 8;
constexpr int kChunk = kThreads * kItems;  // 2048 sorted elements per workgroup
constexpr int kMaxClasses = 64;

// softmax(row)[j] == expf(row[j] - m) / s; the row is re-read from L1 instead of being held in a runtime-indexed
// register array (which the compiler would put in scratch)
__device__ __forceinline__ void softmax_stats(const float* __restrict__ row, int c, float* m_out, float* s_out) {
    float m = row[0];
    for (int j = 1; j < c; ++j) m = fmaxf(m, row[j]);
    float s = 0.f;
    for (int j = 0; j < c; ++j) s += expf(row[j] - m);
    *m_out = m;
    *s_out = s;
}

// cross-entropy of one row given its softmax statistics: log-sum-exp, and whether the row is counted
__device__ __forceinline__ bool ce_row(const float* __restrict__ row, int c, int64_t y, int64_t ignore_index,
                                       float keep_thresh, float m, float s, float* lse_out) {
    *lse_out = m + logf(s);
    bool counted = y != ignore_index && y >= 0 && y < c;
    if (counted && keep_thresh > 0.f) counted = expf(row[y] - m) / s < keep_thresh;  // softmax(x)[y] < keep_thresh
    return counted;
}

// mean over the counted rows from the row pass's per-workgroup partials part[nblocks][2]; valid in thread 0
__device__ __forceinline__ void ce_mean(const float* __restrict__ part, int nblocks, float* mean_out, float* count_out) {
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    block_sum<kThreads>(a, b);  // valid in thread 0
    *mean_out = b > 0.f ? a / b : 0.f;
    *count_out = b;
}

// d CE / d logit of one element: lse is +inf on rows that are not counted
__device__ __forceinline__ float ce_grad(float x, float lse, bool is_label, float scale) {
    float g = 0.f;
    if (lse != INFINITY) g = (expf(x - lse) - (is_label ? 1.f : 0.f)) * scale;
    return g;
}

// Lovasz error of (row, class j): |[label == j] - p_j|, 0 on rows with an ignored label (they sort behind every positive
// error and weigh 0).  Errors are in [0, 1]: their bit patterns order like their values and stay below 2^30.
__device__ __forceinline__ uint32_t lovasz_err_bits(const float* __restrict__ row, int j, float m, float s, bool valid,
                                                    bool fg) {
    const float err = valid ? fabsf((fg ? 1.f : 0.f) - expf(row[j] - m) / s) : 0.f;
    return __float_as_uint(err);
}

// foreground count of chunk `chunk` of a sorted segment v[0, n); valid in thread 0
__device__ __forceinline__ int lovasz_chunk_count(const uint32_t* __restrict__ v, int n, int chunk) {
    int cnt = 0;
    const int base = chunk * kChunk + threadIdx.x * kItems;
    for (int j = 0; j < kItems; ++j)
        if (base + j < n) cnt += (int)(v[base + j] >> 31);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, SEG3D_WAVE);
    __shared__ int red[kThreads / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    int t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / 64; ++w) t += red[w];
    return t;
}

// one wave: exclusive scan of a segment's chunk counts, returns the segment's foreground count (all lanes)
__device__ __forceinline__ int lovasz_segment_offsets(const int* __restrict__ chunk_cnt, int nchunks,
                                                      int* __restrict__ chunk_off) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int t0 = 0; t0 < nchunks; t0 += 64) {
        const int i = t0 + lane;
        const int v = i < nchunks ? chunk_cnt[i] : 0;
        const int inc = wave_scan_inclusive(v, lane);
        if (i < nchunks) chunk_off[i] = carry + inc - v;
        carry += __shfl(inc, 63, SEG3D_WAVE);
    }
    return carry;
}

// One chunk of one sorted segment (keys / vals point at the segment, n elements): running foreground count -> jaccard(k)
// - jaccard(k-1) in the reference's float32 arithmetic, coef[row][cls] = d loss_cls / d p_cls scattered back, and the
// chunk's partial dot with the sorted errors (returned in thread 0).  err_mask: the key bits that hold the error.
__device__ __forceinline__ float lovasz_chunk_grad(const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ vals, uint32_t err_mask, int n, int c,
                                                   int cls, int chunk, int chunk_before, int total,
                                                   float* __restrict__ coef /*[rows][c]*/) {
    const int base = chunk * kChunk + threadIdx.x * kItems;
    uint32_t v[kItems];
    float err[kItems];
    int mine = 0;
    for (int j = 0; j < kItems; ++j) {
        const bool in = base + j < n;
        v[j] = in ? vals[base + j] : 0u;
        err[j] = in ? __uint_as_float((uint32_t)keys[base + j] & err_mask) : 0.f;
        mine += (int)(v[j] >> 31);
    }
    // exclusive scan of the per-thread foreground counts over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, SEG3D_WAVE);
        if (lane >= off) inc += o;
    }
    __shared__ int wsum[kThreads / 64];
    __shared__ float wdot[kThreads / 64];
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = chunk_before + inc - mine;
    for (int w = 0; w < wave; ++w) before += wsum[w];

    const float gts = (float)total;
    float dot = 0.f;
    int cum = before;
    for (int j = 0; j < kItems; ++j) {
        const int k = base + j;
        if (k >= n) break;
        const int fg = (int)(v[j] >> 31);
        const int cum_prev = cum;
        cum += fg;
        // lovasz_grad, lovasz_loss.py:17-25: jaccard = 1 - (gts - cumsum(gt)) / (gts + cumsum(1 - gt)), then differences
        float g = 1.f - (gts - (float)cum) / (gts + (float)(k + 1 - cum));
        if (k > 0) g -= 1.f - (gts - (float)cum_prev) / (gts + (float)(k - cum_prev));
        dot += err[j] * g;
        // d|fg - p| / dp: -1 on foreground rows, +1 on background rows, 0 where the error is exactly 0 (torch abs')
        const float sgn = err[j] == 0.f ? 0.f : (fg ? -1.f : 1.f);
        coef[(int64_t)(v[j] & 0x7FFFFFFFu) * c + cls] = sgn * g;
    }
    for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, SEG3D_WAVE);
    if (lane == 0) wdot[wave] = dot;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / 64; ++w) t += wdot[w];
    return t;
}

// Class selection, weights and mean of one head; part / total are indexed by sorted segment (seg = c - 1 - cls: the sort
// is descending on the class bits).  Called by a whole workgroup of >= c threads; thread 0 writes
// stats[0] = loss, stats[1] = number of classes averaged, stats[2 + cls] = d loss / d loss_cls.
__device__ __forceinline__ void lovasz_head_finalize(const float* __restrict__ part, const int* __restrict__ total, int c,
                                                     int nchunks, int mode, const int32_t* __restrict__ include,
                                                     const float* __restrict__ class_weight, float* __restrict__ stats) {
    __shared__ float loss_c[kMaxClasses];
    __shared__ float w_c[kMaxClasses];
    const int cls = threadIdx.x;
    if (cls < c) {
        const int seg = c - 1 - cls;
        float s = 0.f;
        for (int i = 0; i < nchunks; ++i) s += part[seg * nchunks + i];
        bool use = mode == 0 ? total[seg] > 0 : true;  // 'present' (lovasz_loss.py:143-144) | 'all'
        if (include) use = include[cls] != 0;          // explicit class list: no presence test (lovasz_loss.py:140)
        const float w = use ? (class_weight ? class_weight[cls] : 1.f) : 0.f;
        loss_c[cls] = use ? s * w : 0.f;
        w_c[cls] = use ? w : -1.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        int used = 0;
        for (int j = 0; j < c; ++j)
            if (w_c[j] >= 0.f) {
                sum += loss_c[j];
                ++used;
            }
        stats[0] = used ? sum / (float)used : 0.f;
        stats[1] = (float)used;
        for (int j = 0; j < c; ++j) stats[2 + j] = (w_c[j] >= 0.f && used) ? w_c[j] / (float)used : 0.f;
    }
}

// softmax backward of the Lovasz term on one row: dot = <p, dp> with dp_j = coef[j] * cscale[j] * g
__device__ __forceinline__ float lovasz_row_dot(const float* __restrict__ row, const float* __restrict__ cf,
                                                const float* __restrict__ cscale, int c, float m, float s, float g) {
    float dot = 0.f;
    for (int j = 0; j < c; ++j) dot += expf(row[j] - m) / s * (cf[j] * cscale[j] * g);
    return dot;
}

__device__ __forceinline__ float lovasz_grad_elem(float x, float cf, float cscale, float m, float s, float g, float dot) {
    return expf(x - m) / s * (cf * cscale * g - dot);
}

static inline int class_bits(int c) {
    int b = 0;
    while ((1 << b) < c) ++b;
    return b;
}

}  // namespace crit
