// Evaluation path: test-time-augmentation views, softmax accumulation over views, argmax + confusion matrix.
// Reference: seg3d/datasets/transforms/test_time_aug.py:15-35 (MultiScaleFlipAug), tools/eval.py:35-64 (the eval loop:
// F.softmax per view, torch.stack + mean, argmax), seg3d/core/evaluation/iou_metric.py:21-53 (fast_hist / add).
//
// MI355X design: the reference builds 36 views per frame on the host and runs 36 batch-1 forwards; here the views of a
// frame are written in one launch straight into the collated [V*N, 1+D] layout the device voxelizer reads, the softmax
// of every forward is folded into a running fp32 sum (one rounded add per view, in view order, so any split of the views
// into forwards gives the same bits), and the argmax feeds a per-workgroup LDS histogram instead of a host bincount.
// All three are memory-bound streaming kernels; none allocates or synchronises (hipGraph-capturable).
#include "common.hpp"

// the TTA recipe is two IEEE products and one sum per rotated coordinate, as the reference's float32 torch.matmul rounds
// them; a fused multiply-add would change the last bit against the host twin
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDim = 16;  // point columns handled by the views kernel (the shipped configs use 6)

// ------------------------------------------------------------------------------------------ (a) TTA views
// test_time_aug.py:26-31 with transform_utils.py:11-32: scale the xyz, rotate by points @ R(angle) with
// R = [[c, s, 0], [-s, c, 0], [0, 0, 1]], then flip_x negates y and flip_y negates x.  Shared by the kernel and the host
// twin, so both round the same operations.
__host__ __device__ __forceinline__ void tta_point(const seg3d_tta_view& w, float x, float y, float z, float* o) {
    x = x * w.scale;
    y = y * w.scale;
    z = z * w.scale;
    float xr = x * w.cos_a + y * (-w.sin_a);
    float yr = x * w.sin_a + y * w.cos_a;
    if (w.flip_x) yr = -yr;
    if (w.flip_y) xr = -xr;
    o[0] = xr;
    o[1] = yr;
    o[2] = z;
}

__host__ __device__ __forceinline__ float view_tag(const seg3d_tta_table& t, uint32_t v) {
    return (float)(t.batch_period > 0 ? v % (uint32_t)t.batch_period : v);
}

// one thread = four consecutive output rows g0..g0+3 of the [V*N, 1+D] result: their 4*(1+D) floats start on a 16-B
// boundary for every D, so the stores are (1+D) float4; the four input rows are read as D float4 when they are four
// consecutive points starting at a multiple of 4 (always, for N % 4 == 0), element by element otherwise
template <int D>
__global__ __launch_bounds__(kThreads) void tta_views_kernel(const float* __restrict__ pts, int64_t n, int64_t total,
                                                             seg3d_tta_table tab, int vec, float* __restrict__ out) {
    constexpr int W = D + 1;
    const int64_t g0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (g0 >= total) return;
    const uint32_t nu = (uint32_t)n, v0 = (uint32_t)g0 / nu, i0 = (uint32_t)g0 - v0 * nu;  // V*N <= INT32_MAX
    const bool full = g0 + 4 <= total;
    float in[4 * D];
    if (vec && full && i0 + 4 <= n && (i0 & 3) == 0) {
        const float4* p4 = reinterpret_cast<const float4*>(pts + (int64_t)i0 * D);
#pragma unroll
        for (int q = 0; q < D; ++q) {
            const float4 f = p4[q];
            in[4 * q] = f.x;
            in[4 * q + 1] = f.y;
            in[4 * q + 2] = f.z;
            in[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t i = (i0 + r) % nu;  // a group that runs over the end of a view continues in the next
            const bool ok = g0 + r < total;
#pragma unroll
            for (int c = 0; c < D; ++c) in[r * D + c] = ok ? pts[(int64_t)i * D + c] : 0.f;
        }
    }
    float o[4 * W];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t v = v0 + (i0 + r) / nu;
        const int vi = (int)(v < (uint32_t)tab.n_views ? v : (uint32_t)tab.n_views - 1);  // rows past the end are computed, never stored
        o[r * W] = view_tag(tab, v);
        tta_point(tab.views[vi], in[r * D], in[r * D + 1], in[r * D + 2], &o[r * W + 1]);
#pragma unroll
        for (int c = 3; c < D; ++c) o[r * W + 1 + c] = in[r * D + c];
    }
    if (vec && full) {
        float4* o4 = reinterpret_cast<float4*>(out + g0 * W);
#pragma unroll
        for (int q = 0; q < W; ++q) o4[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    } else {
        for (int r = 0; r < 4; ++r) {
            if (g0 + r >= total) break;
#pragma unroll
            for (int c = 0; c < W; ++c) out[(g0 + r) * W + c] = o[r * W + c];
        }
    }
}

bool table_ok(const seg3d_tta_table* t) {
    if (!t || t->n_views < 1 || t->n_views > SEG3D_TTA_MAX_VIEWS || t->batch_period < 0) return false;
    for (int v = 0; v < t->n_views; ++v) {
        const seg3d_tta_view& w = t->views[v];
        if ((w.flip_x != 0 && w.flip_x != 1) || (w.flip_y != 0 && w.flip_y != 1)) return false;
    }
    return true;
}

bool views_args_ok(const float* points, int64_t n, int32_t dim, const seg3d_tta_table* t, const float* out) {
    if (n < 0 || dim < 3 || dim > kMaxDim || !table_ok(t)) return false;
    if (n > (int64_t)INT32_MAX / t->n_views) return false;  // V*N rows indexed in int64, bounded to keep (1+D)*V*N sane
    if (n > 0 && (!points || !out)) return false;
    return true;
}

template <int D>
void launch_views(const float* points, int64_t n, const seg3d_tta_table& t, float* out, hipStream_t st) {
    const int64_t total = n * t.n_views;
    const int vec = ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const unsigned nb = (unsigned)ceil_div64(ceil_div64(total, 4), kThreads);
    hipLaunchKernelGGL(tta_views_kernel<D>, dim3(nb), dim3(kThreads), 0, st, points, n, total, t, vec, out);
}

// ------------------------------------------------------------------------------------------ (b) softmax accumulate
// One wave per workgroup, 64 consecutive points per wave.  The accumulator rows of those points (64*C contiguous floats,
// 88 B rows at C = 22: not 16-B aligned) and, view by view, the matching logits rows are staged through LDS with 16-B
// loads over the aligned cover of the span; each lane then works on its own row.  Edges of the span that share a float4
// with a neighbouring wave are written element by element (no store ever touches another wave's rows).
constexpr int kSmRows = 64;

__device__ __forceinline__ void stage_span(const float* __restrict__ g, int64_t e0, int64_t e1, int64_t limit, bool vec,
                                           float* lds, int64_t a0) {
    // lds[j] = g[a0 + j] for a0 + j in [e0, e1) (a0 = e0 rounded down to a multiple of 4)
    if (vec) {
        const int64_t q0 = a0 >> 2, q1 = (e1 + 3) >> 2;
        for (int64_t q = q0 + threadIdx.x; q < q1; q += kSmRows) {
            float* d = lds + (q - q0) * 4;
            if (q * 4 + 4 <= limit) {
                const float4 f = reinterpret_cast<const float4*>(g)[q];
                d[0] = f.x;
                d[1] = f.y;
                d[2] = f.z;
                d[3] = f.w;
            } else {
                for (int j = 0; j < 4; ++j)
                    if (q * 4 + j < limit) d[j] = g[q * 4 + j];
            }
        }
    } else {
        for (int64_t e = e0 + threadIdx.x; e < e1; e += kSmRows) lds[e - a0] = g[e];
    }
}

__global__ __launch_bounds__(kSmRows) void softmax_accumulate_kernel(const float* __restrict__ logits, int64_t n, int k_views,
                                                                     int c, int first, int vec, float* __restrict__ acc) {
    extern __shared__ float smem[];
    const int span = kSmRows * c + 8;  // + alignment slack at both ends
    float* lacc = smem;
    float* llog = smem + span;
    const int64_t p0 = (int64_t)blockIdx.x * kSmRows;
    const int rows = (int)(n - p0 < kSmRows ? n - p0 : kSmRows);
    const int lane = threadIdx.x;
    const int64_t ae0 = p0 * c, ae1 = ae0 + (int64_t)rows * c, aa0 = ae0 & ~(int64_t)3;
    if (!first) stage_span(acc, ae0, ae1, n * c, vec, lacc, aa0);
    const int64_t total = (int64_t)k_views * n * c;
    for (int k = 0; k < k_views; ++k) {
        const int64_t le0 = ((int64_t)k * n + p0) * c, le1 = le0 + (int64_t)rows * c, la0 = le0 & ~(int64_t)3;
        stage_span(logits, le0, le1, total, vec, llog, la0);
        __syncthreads();
        if (lane < rows) {
            float* l = llog + (le0 - la0) + lane * c;
            float* a = lacc + (ae0 - aa0) + lane * c;
            float m = l[0];
            for (int j = 1; j < c; ++j) m = l[j] > m ? l[j] : m;
            float s = 0.f;
            for (int j = 0; j < c; ++j) {
                const float e = expf(l[j] - m);
                l[j] = e;
                s = s + e;
            }
            const bool over = first && k == 0;
            for (int j = 0; j < c; ++j) {
                const float p = l[j] / s;
                a[j] = over ? p : a[j] + p;
            }
        }
        __syncthreads();
    }
    // write back: interior float4 aligned, the (at most two) partial float4 at the ends element by element
    const float* src = lacc + (ae0 - aa0);
    if (vec) {
        const int64_t q0 = (ae0 + 3) >> 2, q1 = ae1 >> 2;  // float4 fully inside [ae0, ae1)
        for (int64_t q = q0 + lane; q < q1; q += kSmRows) {
            const float* s4 = lacc + (q * 4 - aa0);
            reinterpret_cast<float4*>(acc)[q] = make_float4(s4[0], s4[1], s4[2], s4[3]);
        }
        const int64_t head_end = q0 * 4 < ae1 ? q0 * 4 : ae1;
        for (int64_t e = ae0 + lane; e < head_end; e += kSmRows) acc[e] = src[e - ae0];
        const int64_t tail_beg = q1 * 4 > ae0 ? q1 * 4 : ae0;
        if (tail_beg >= head_end)
            for (int64_t e = tail_beg + lane; e < ae1; e += kSmRows) acc[e] = src[e - ae0];
    } else {
        for (int64_t e = ae0 + lane; e < ae1; e += kSmRows) acc[e] = src[e - ae0];
    }
}

// ------------------------------------------------------------------------------------------ (c) argmax + confusion
constexpr int kHistThreads = 256;
constexpr int kMaxHistBlocks = 2048;

// torch.argmax / numpy argmax: the first maximum wins; a NaN counts as the maximum and the first NaN wins
__device__ __forceinline__ int row_argmax(const float* __restrict__ row, int c, float div) {
    float best = row[0];
    if (div > 0.f) best = best / div;
    if (best != best) return 0;
    int idx = 0;
    for (int j = 1; j < c; ++j) {
        float v = row[j];
        if (div > 0.f) v = v / div;  // torch.mean: the correctly rounded quotient, not a product with 1/V
        if (v != v) return j;
        if (v > best) {
            best = v;
            idx = j;
        }
    }
    return idx;
}

__global__ __launch_bounds__(kHistThreads) void argmax_confusion_kernel(const float* __restrict__ scores,
                                                                        const int64_t* __restrict__ pred_in, int64_t n, int c,
                                                                        float div, const void* __restrict__ labels,
                                                                        int label_bytes, int64_t* __restrict__ pred,
                                                                        unsigned long long* __restrict__ hist) {
    __shared__ uint32_t lh[SEG3D_ARGMAX_MAX_CLASSES * SEG3D_ARGMAX_MAX_CLASSES];
    const int cc = c * c;
    if (hist) {
        for (int b = threadIdx.x; b < cc; b += kHistThreads) lh[b] = 0u;
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * kHistThreads;
    for (int64_t i = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; i < n; i += stride) {
        int64_t p;
        if (pred_in) {
            p = pred_in[i];
        } else {
            p = row_argmax(scores + i * c, c, div);
            if (pred) pred[i] = p;
        }
        if (hist) {
            const int64_t g = label_bytes == 1 ? (int64_t)static_cast<const uint8_t*>(labels)[i]
                                               : static_cast<const int64_t*>(labels)[i];
            // iou_metric.py:33 masks labels outside [0, C) (ignore index 255); a given pred outside [0, C) has no bin
            if (g >= 0 && g < c && p >= 0 && p < c) atomicAdd(&lh[g * c + p], 1u);
        }
    }
    if (hist) {
        __syncthreads();
        for (int b = threadIdx.x; b < cc; b += kHistThreads) {
            const uint32_t v = lh[b];
            if (v) atomicAdd(&hist[b], (unsigned long long)v);
        }
    }
}

}  // namespace

extern "C" {

int seg3d_tta_views_f32(const float* points, int64_t n_points, int32_t dim, const seg3d_tta_table* table, float* out,
                        void* stream) {
    if (!views_args_ok(points, n_points, dim, table, out)) return SEG3D_EINVAL;
    if (n_points == 0) return SEG3D_OK;
    const seg3d_tta_table t = *table;  // by value into the kernel arguments: no copy to the device
    hipStream_t st = as_stream(stream);
    switch (dim) {
#define SEG3D_VIEWS_CASE(d) \
    case d: launch_views<d>(points, n_points, t, out, st); break;
        SEG3D_VIEWS_CASE(3) SEG3D_VIEWS_CASE(4) SEG3D_VIEWS_CASE(5) SEG3D_VIEWS_CASE(6) SEG3D_VIEWS_CASE(7)
        SEG3D_VIEWS_CASE(8) SEG3D_VIEWS_CASE(9) SEG3D_VIEWS_CASE(10) SEG3D_VIEWS_CASE(11) SEG3D_VIEWS_CASE(12)
        SEG3D_VIEWS_CASE(13) SEG3D_VIEWS_CASE(14) SEG3D_VIEWS_CASE(15) SEG3D_VIEWS_CASE(16)
#undef SEG3D_VIEWS_CASE
        default: return SEG3D_EINVAL;
    }
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_tta_views_host_f32(const float* points, int64_t n_points, int32_t dim, const seg3d_tta_table* table,
                             float* out) {
    if (!views_args_ok(points, n_points, dim, table, out)) return SEG3D_EINVAL;
    const seg3d_tta_table& t = *table;
    const int w = dim + 1;
    for (int64_t v = 0; v < t.n_views; ++v) {
        for (int64_t i = 0; i < n_points; ++i) {
            const float* p = points + i * dim;
            float* o = out + (v * n_points + i) * w;
            o[0] = view_tag(t, (uint32_t)v);
            tta_point(t.views[v], p[0], p[1], p[2], o + 1);
            for (int c = 3; c < dim; ++c) o[1 + c] = p[c];
        }
    }
    return SEG3D_OK;
}

int seg3d_softmax_accumulate_f32(const float* logits, int64_t n_points, int32_t n_views, int32_t c, int32_t first,
                                 float* acc, void* stream) {
    if (n_points < 0 || n_views < 1 || n_views > SEG3D_TTA_MAX_VIEWS || c < 1 || c > SEG3D_ARGMAX_MAX_CLASSES ||
        (first != 0 && first != 1))
        return SEG3D_EINVAL;
    if (n_points > (int64_t)INT32_MAX / n_views) return SEG3D_EINVAL;  // K*N rows
    if (n_points == 0) return SEG3D_OK;
    if (!logits || !acc) return SEG3D_EINVAL;
    const int vec = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0;
    const size_t lds = (size_t)2 * (kSmRows * c + 8) * sizeof(float);
    hipLaunchKernelGGL(softmax_accumulate_kernel, dim3((unsigned)ceil_div64(n_points, kSmRows)), dim3(kSmRows), lds,
                       as_stream(stream), logits, n_points, (int)n_views, (int)c, (int)first, vec, acc);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_argmax_confusion(const float* scores, const int64_t* pred_in, int64_t n_points, int32_t c, int32_t n_views,
                           const void* labels, int32_t label_bytes, int64_t* pred, int64_t* hist, void* stream) {
    if (n_points < 0 || c < 1 || c > SEG3D_ARGMAX_MAX_CLASSES || n_views < 0) return SEG3D_EINVAL;
    if (n_points == 0) return SEG3D_OK;  // (empty tensors hand over null pointers)
    if ((scores != nullptr) == (pred_in != nullptr)) return SEG3D_EINVAL;  // exactly one source of predictions
    if (pred_in && (pred || n_views)) return SEG3D_EINVAL;
    if (hist && (!labels || (label_bytes != 1 && label_bytes != 8))) return SEG3D_EINVAL;
    if (!pred && !hist) return SEG3D_EINVAL;  // nothing to produce
    const int64_t want = ceil_div64(n_points, kHistThreads);
    const unsigned nb = (unsigned)(want < kMaxHistBlocks ? want : kMaxHistBlocks);
    hipLaunchKernelGGL(argmax_confusion_kernel, dim3(nb), dim3(kHistThreads), 0, as_stream(stream), scores, pred_in,
                       n_points, (int)c, (float)n_views, labels, (int)label_bytes, pred,
                       reinterpret_cast<unsigned long long*>(hist));
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

}  // extern "C"
