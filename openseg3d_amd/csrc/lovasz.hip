// Lovasz-softmax on device (seg3d/models/losses/lovasz_loss.py:13-26 lovasz_grad, :118-158
// lovasz_softmax_flat, :268-290 LovaszLoss.forward with the defaults build_criterion uses: multi_class, per_image
// False, ignore_index 255).  The reference loops over the C classes and for each one sorts all N errors, gathers,
// runs two cumsums and a dot (C x ~12 launches, three times per training step).  Here every class is handled at once:
//
//   lovasz_keys   one thread per row: softmax, then for every class c the pair
//                   key = c << 32 | bits(|[label == c] - p_c|)      (errors are in [0, 1]: bit order == value order)
//                   val = row | [label == c] << 31                  (rows with an ignored label: error 0, fg 0 -- they
//                                                                    sort behind every positive error and weigh 0)
//   rocprim::radix_sort_pairs_desc over the low 32 + log2(C) key bits: class C-1-c occupies [c*n, (c+1)*n), errors
//                 descending inside it (one full-chip sort instead of C single-segment sorts)
//   lovasz_count / lovasz_offsets   foreground count of every 2048-element chunk, exclusive scan per class, totals
//   lovasz_grad   per chunk: running foreground count -> jaccard(k) - jaccard(k-1) in the reference's float32
//                 arithmetic, partial dot with the sorted errors, and coef[row][c] = d loss_c / d p_c scattered back
//   lovasz_finalize  fixed-order sum of the chunk partials, class selection ('present' | 'all' | mask), weights, mean
// Backward is one pass: dlogits = p * (dp - <p, dp>) with dp_c = coef[row][c] * cscale[c] * g.
// No atomics, no memsets: every workspace word that is read was written by an earlier kernel of the same call.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "criterion_device.hpp"

namespace {

using crit::class_bits;
using crit::kChunk;
using crit::kMaxClasses;
using crit::kThreads;

__global__ __launch_bounds__(kThreads) void lovasz_keys(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                        int n, int c, int64_t ignore_index,
                                                        unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const float* row = x + (int64_t)r * c;
    float m, s;
    crit::softmax_stats(row, c, &m, &s);
    const int64_t y = label[r];
    const bool valid = y != ignore_index;
    for (int j = 0; j < c; ++j) {
        const bool fg = valid && y == j;
        const int64_t at = (int64_t)j * n + r;
        keys[at] = ((unsigned long long)j << 32) | crit::lovasz_err_bits(row, j, m, s, valid, fg);
        vals[at] = (uint32_t)r | (fg ? 0x80000000u : 0u);
    }
}

__global__ __launch_bounds__(kThreads) void lovasz_count(const uint32_t* __restrict__ vals, int n, int nchunks,
                                                         int* __restrict__ chunk_cnt /*[c][nchunks]*/) {
    const int seg = blockIdx.y, chunk = blockIdx.x;
    const int t = crit::lovasz_chunk_count(vals + (int64_t)seg * n, n, chunk);
    if (threadIdx.x == 0) chunk_cnt[seg * nchunks + chunk] = t;
}

// one wave per sorted segment: exclusive scan of its chunk counts, total foreground count
__global__ __launch_bounds__(64) void lovasz_offsets(const int* __restrict__ chunk_cnt, int nchunks,
                                                     int* __restrict__ chunk_off, int* __restrict__ total) {
    const int seg = blockIdx.x;
    const int t = crit::lovasz_segment_offsets(chunk_cnt + seg * nchunks, nchunks, chunk_off + seg * nchunks);
    if (threadIdx.x == 0) total[seg] = t;
}

__global__ __launch_bounds__(kThreads) void lovasz_grad(const unsigned long long* __restrict__ keys,
                                                        const uint32_t* __restrict__ vals, int n, int c, int nchunks,
                                                        const int* __restrict__ chunk_off, const int* __restrict__ total,
                                                        float* __restrict__ coef /*[n][c]*/,
                                                        float* __restrict__ part /*[c][nchunks]*/) {
    const int seg = blockIdx.y, chunk = blockIdx.x;
    const int cls = c - 1 - seg;  // descending sort on the class bits
    const int64_t seg0 = (int64_t)seg * n;
    const float t = crit::lovasz_chunk_grad(keys + seg0, vals + seg0, 0xFFFFFFFFu, n, c, cls, chunk,
                                            chunk_off[seg * nchunks + chunk], total[seg], coef);
    if (threadIdx.x == 0) part[seg * nchunks + chunk] = t;
}

// stats[0] = loss, stats[1] = number of classes averaged, stats[2 + cls] = d loss / d loss_cls
__global__ __launch_bounds__(kMaxClasses) void lovasz_finalize(const float* __restrict__ part, const int* __restrict__ total,
                                                               int c, int nchunks, int mode,
                                                               const int32_t* __restrict__ include,
                                                               const float* __restrict__ class_weight,
                                                               float* __restrict__ stats) {
    crit::lovasz_head_finalize(part, total, c, nchunks, mode, include, class_weight, stats);
}

__global__ __launch_bounds__(kThreads) void lovasz_bwd(const float* __restrict__ x, const float* __restrict__ coef,
                                                       const float* __restrict__ stats, const float* __restrict__ gout,
                                                       int n, int c, float* __restrict__ dx) {
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const float* row = x + (int64_t)r * c;
    float m, s;
    crit::softmax_stats(row, c, &m, &s);
    const float g = gout[0];
    const float* cf = coef + (int64_t)r * c;
    const float dot = crit::lovasz_row_dot(row, cf, stats + 2, c, m, s, g);
    float* out = dx + (int64_t)r * c;
    for (int j = 0; j < c; ++j) out[j] = crit::lovasz_grad_elem(row[j], cf[j], stats[2 + j], m, s, g, dot);
}

using Key = unsigned long long;

struct Plan {
    int64_t total;
    int nchunks;
    size_t sort_bytes;
};

bool make_plan(int64_t n, int c, Plan* pl) {
    pl->total = n * c;
    pl->nchunks = (int)ceil_div64(n, kChunk);
    pl->sort_bytes = 0;
    if (pl->total == 0) return true;
    rocprim::double_buffer<Key> k(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs_desc(nullptr, bytes, k, v, (size_t)pl->total, 0u, 32u + class_bits(c)) != hipSuccess)
        return false;
    pl->sort_bytes = bytes;
    return true;
}

}  // namespace

// 0 when the arguments are invalid or no device is visible (the sort's scratch size is asked of rocPRIM, which sizes
// it for the current device).
extern "C" size_t seg3d_lovasz_workspace_bytes(int64_t n, int32_t c) {
    if (n < 0 || c <= 0 || c > kMaxClasses || n * c >= (int64_t)1 << 31) return 0;
    Plan pl;
    if (!make_plan(n, c, &pl)) return 0;
    const size_t t = (size_t)pl.total, cc = (size_t)c * pl.nchunks;
    return 2 * align_up(t * sizeof(Key), 256) + 2 * align_up(t * sizeof(uint32_t), 256) + align_up(pl.sort_bytes, 256) +
           2 * align_up(cc * sizeof(int), 256) + align_up(cc * sizeof(float), 256) + align_up(c * sizeof(int), 256) + 256;
}

extern "C" int seg3d_lovasz_softmax_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c,
                                        int64_t ignore_index, int32_t classes_mode, const int32_t* include,
                                        const float* class_weight, float* coef, float* stats, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (n < 0 || c <= 0 || c > kMaxClasses || n * c >= (int64_t)1 << 31 || !stats || (classes_mode != 0 && classes_mode != 1))
        return SEG3D_EINVAL;
    hipStream_t st = as_stream(stream);
    Plan pl;
    if (!make_plan(n, c, &pl)) return SEG3D_ELAUNCH;
    const size_t need = seg3d_lovasz_workspace_bytes(n, c);
    if (!workspace || need == 0 || workspace_bytes < need) return SEG3D_EWORKSPACE;
    if (n > 0 && (!logits || !labels || !coef)) return SEG3D_EINVAL;
    const size_t t = (size_t)pl.total, cc = (size_t)c * (size_t)(pl.nchunks > 0 ? pl.nchunks : 0);
    WsCarver ws(workspace);
    Key* k0 = ws.take<Key>(t);
    Key* k1 = ws.take<Key>(t);
    uint32_t* v0 = ws.take<uint32_t>(t);
    uint32_t* v1 = ws.take<uint32_t>(t);
    void* sort_tmp = ws.take<char>(pl.sort_bytes);
    int* chunk_cnt = ws.take<int>(cc);
    int* chunk_off = ws.take<int>(cc);
    float* part = ws.take<float>(cc);
    int* total = ws.take<int>((size_t)c);
    const int ni = (int)n;
    if (n > 0) {
        hipLaunchKernelGGL(lovasz_keys, dim3((unsigned)ceil_div64(n, kThreads)), dim3(kThreads), 0, st, logits, labels, ni, c,
                           ignore_index, k0, v0);
        SEG3D_CHECK_LAUNCH();
        rocprim::double_buffer<Key> kb(k0, k1);
        rocprim::double_buffer<uint32_t> vb(v0, v1);
        size_t bytes = pl.sort_bytes;
        SEG3D_CHECK_HIP(rocprim::radix_sort_pairs_desc(sort_tmp, bytes, kb, vb, t, 0u, 32u + class_bits(c), st));
        const dim3 grid((unsigned)pl.nchunks, (unsigned)c);
        hipLaunchKernelGGL(lovasz_count, grid, dim3(kThreads), 0, st, vb.current(), ni, pl.nchunks, chunk_cnt);
        SEG3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(lovasz_offsets, dim3((unsigned)c), dim3(64), 0, st, chunk_cnt, pl.nchunks, chunk_off, total);
        SEG3D_CHECK_LAUNCH();
        hipLaunchKernelGGL(lovasz_grad, grid, dim3(kThreads), 0, st, kb.current(), vb.current(), ni, c, pl.nchunks, chunk_off,
                           total, coef, part);
        SEG3D_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(lovasz_offsets, dim3((unsigned)c), dim3(64), 0, st, chunk_cnt, 0, chunk_off, total);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(lovasz_finalize, dim3(1), dim3(kMaxClasses), 0, st, part, total, c, pl.nchunks, classes_mode, include,
                       class_weight, stats);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_lovasz_softmax_bwd(const float* logits, const float* coef, const float* stats, const float* grad_out,
                                        int64_t n, int32_t c, float* dlogits, void* stream) {
    if (n < 0 || c <= 0 || c > kMaxClasses || n * c >= (int64_t)1 << 31 || !stats || !grad_out) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    if (!logits || !coef || !dlogits) return SEG3D_EINVAL;
    hipLaunchKernelGGL(lovasz_bwd, dim3((unsigned)ceil_div64(n, kThreads)), dim3(kThreads), 0, as_stream(stream), logits, coef,
                       stats, grad_out, (int)n, c, dlogits);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}
