// Frame assembly: the multi-sweep merge in front of the voxelizer and the range-image write-back behind the head.
// Reference: seg3d/datasets/waymo_dataset.py:145-154 (load_points: zeroed range column, tanh of the intensity),
// :156-202 (load_points_from_sweeps: per history sweep `points @ R.T`, `+= t`, the time-lag column, np.concatenate),
// seg3d/utils/data_utils.py:6-15 (load_data_to_gpu's `.float()`), seg3d/utils/submission.py:27-41 (construct_seg_frame:
// a Python loop over every point that writes `pred + 1` into two range images).
//
// MI355X design.  The merge moves 50-100 B per row and does a dozen flops on it, so it is one streaming kernel for all
// sweeps of a frame: the sweep table travels by value among the kernel arguments, a workgroup owns 256 consecutive
// OUTPUT rows (which may straddle sweeps), stages their source rows through LDS with lane-consecutive loads (a raw row
// is 24-128 B at a stride of up to 120 B: one row per lane would be a strided access), lets one lane finish one row in
// LDS, and streams the tile out lane-consecutively once per requested layout.  The range images are an atomic max of a
// packed (row index + 1, label + 1) word per pixel followed by an unpack pass: integer-exact, the highest row index
// wins whatever the launch geometry.  Nothing here allocates or synchronises; no float atomics.
// Each device entry has a host twin below it: plain C++ that makes no HIP call and shares the per-row recipe.
#include <math.h>
#include <string.h>

#include "common.hpp"

// the recipe is a fixed sequence of IEEE products and sums, each rounded as numpy rounds it; a fused multiply-add would
// change the last bit against the host twin and the reference
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 256;
constexpr int kMaxDim = 16;
constexpr int kMinDim = 5;
constexpr int kMaxBlocks = 512;  // two workgroups per CU; larger frames loop over tiles

struct SweepStarts {
    int64_t start[SEG3D_FRAME_MAX_SWEEPS + 1];  // first output row of every sweep, then the total
};

__host__ __device__ __forceinline__ float tanh_t(float v) { return tanhf(v); }
__host__ __device__ __forceinline__ double tanh_t(double v) { return tanh(v); }

// One row, in place, in the rows' own dtype T -- waymo_dataset.py:151-153 and :196-198 in their order:
// column 3 = T(lag) (the range column is zeroed, then `ts - sweep_ts` is stored; the current sweep has lag 0),
// column 4 = tanh in T, then for a history sweep `xyz @ R.T` in double rounded to T (numpy assigns the product back into
// the array) and `+= t` rounded to T again.  Without the flag x, y, z are left bit for bit.
template <typename T>
__host__ __device__ __forceinline__ void frame_row(const seg3d_sweep& s, T* r) {
    r[3] = (T)s.lag;
    r[4] = tanh_t(r[4]);
    if (s.transform) {
        const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double* m = s.matrix + 4 * k;
            const T p = (T)((x * m[0] + y * m[1]) + z * m[2]);
            r[k] = (T)((double)p + m[3]);
        }
    }
}

__host__ __device__ __forceinline__ int sweep_of(const SweepStarts& st, int n_sweeps, int64_t g) {
    int s = 0;
    while (s + 1 < n_sweeps && g >= st.start[s + 1]) ++s;  // empty sweeps are stepped over
    return s;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void frame_assemble_kernel(seg3d_sweep_table tab, SweepStarts st, int dim,
                                                                  T* __restrict__ out_rows, float* __restrict__ out_f32,
                                                                  float* __restrict__ out_collated, float batch_id) {
    __shared__ T tile[kTileRows * kMaxDim];
    __shared__ uint8_t tile_sweep[kTileRows];
    const int64_t total = st.start[tab.n_sweeps];
    const int t = threadIdx.x;
    const int w = dim + 1;
    for (int64_t p0 = (int64_t)blockIdx.x * kTileRows; p0 < total; p0 += (int64_t)gridDim.x * kTileRows) {
        const int rows = (int)(total - p0 < kTileRows ? total - p0 : kTileRows);
        if (t < rows) tile_sweep[t] = (uint8_t)sweep_of(st, tab.n_sweeps, p0 + t);
        __syncthreads();
        for (int e = t; e < rows * dim; e += kThreads) {
            const int r = e / dim, c = e - r * dim;
            const int s = tile_sweep[r];
            const T* src = static_cast<const T*>(tab.sweeps[s].rows);
            tile[e] = src[(p0 + r - st.start[s]) * tab.sweeps[s].stride + c];
        }
        __syncthreads();
        if (t < rows) frame_row<T>(tab.sweeps[tile_sweep[t]], &tile[t * dim]);
        __syncthreads();
        if (out_rows)
            for (int e = t; e < rows * dim; e += kThreads) out_rows[p0 * dim + e] = tile[e];
        if (out_f32)
            for (int e = t; e < rows * dim; e += kThreads) out_f32[p0 * dim + e] = (float)tile[e];
        if (out_collated)
            for (int e = t; e < rows * w; e += kThreads) {
                const int r = e / w, c = e - r * w;
                out_collated[p0 * w + e] = c == 0 ? batch_id : (float)tile[r * dim + c - 1];
            }
        __syncthreads();
    }
}

// fills the starts; false = a bad table
bool table_ok(const seg3d_sweep_table* tab, int32_t dim, int32_t point_bytes, SweepStarts* st) {
    if (!tab || tab->n_sweeps < 1 || tab->n_sweeps > SEG3D_FRAME_MAX_SWEEPS) return false;
    if (dim < kMinDim || dim > kMaxDim || (point_bytes != 4 && point_bytes != 8)) return false;
    int64_t total = 0;
    for (int s = 0; s < tab->n_sweeps; ++s) {
        const seg3d_sweep& e = tab->sweeps[s];
        if (e.n_rows < 0 || e.stride < dim || (e.n_rows > 0 && !e.rows) || (e.transform != 0 && e.transform != 1))
            return false;
        if (e.n_rows > (int64_t)INT32_MAX || e.stride > 4096) return false;
        st->start[s] = total;
        total += e.n_rows;
    }
    for (int s = tab->n_sweeps; s <= SEG3D_FRAME_MAX_SWEEPS; ++s) st->start[s] = total;
    return total <= (int64_t)INT32_MAX;  // the voxelizer's row ids are int32
}

template <typename T>
void assemble_host(const seg3d_sweep_table& tab, int dim, T* out_rows, float* out_f32, float* out_collated,
                   float batch_id) {
    int64_t g = 0;
    T row[kMaxDim];
    for (int s = 0; s < tab.n_sweeps; ++s) {
        const seg3d_sweep& e = tab.sweeps[s];
        const T* src = static_cast<const T*>(e.rows);
        for (int64_t i = 0; i < e.n_rows; ++i, ++g) {
            for (int c = 0; c < dim; ++c) row[c] = src[i * e.stride + c];
            frame_row<T>(e, row);
            if (out_rows)
                for (int c = 0; c < dim; ++c) out_rows[g * dim + c] = row[c];
            if (out_f32)
                for (int c = 0; c < dim; ++c) out_f32[g * dim + c] = (float)row[c];
            if (out_collated) {
                out_collated[g * (dim + 1)] = batch_id;
                for (int c = 0; c < dim; ++c) out_collated[g * (dim + 1) + 1 + c] = (float)row[c];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ range images
// pixel word: (point index + 1) << 8 | (label + 1); 0 = no point.  The maximum over a pixel's points is the point with
// the highest index: construct_seg_frame's loop (submission.py:33-41) lets the last point win.
__host__ __device__ __forceinline__ int64_t pred_at(const void* pred, int pred_bytes, int64_t i) {
    return pred_bytes == 1 ? (int64_t) static_cast<const uint8_t*>(pred)[i] : static_cast<const int64_t*>(pred)[i];
}

// 0: skipped (no return index of the top lidar), 1: a pixel to write, 2: counted as out of the image
__host__ __device__ __forceinline__ int ri_target(const int32_t* ri, int64_t label, int rows, int cols, int n_classes,
                                                  int64_t* pixel) {
    const int32_t col = ri[0], row = ri[1], ret = ri[2];
    if (ret != 0 && ret != 1) return 0;
    if (row < 0 || row >= rows || col < 0 || col >= cols || label < 0 || label >= n_classes) return 2;
    *pixel = ((int64_t)ret * rows + row) * cols + col;
    return 1;
}

__global__ __launch_bounds__(kThreads) void ri_scatter_kernel(const void* __restrict__ pred, int pred_bytes,
                                                              const int32_t* __restrict__ ri, int64_t n, int rows, int cols,
                                                              int n_classes, unsigned long long* __restrict__ words,
                                                              int32_t* __restrict__ n_outside) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t label = pred_at(pred, pred_bytes, i);
    int64_t pixel = 0;
    const int what = ri_target(ri + 3 * i, label, rows, cols, n_classes, &pixel);
    if (what == 1)
        atomicMax(&words[pixel], ((unsigned long long)(i + 1) << 8) | (unsigned long long)(label + 1));
    else if (what == 2)
        atomicAdd(n_outside, 1);
}

__global__ __launch_bounds__(kThreads) void ri_unpack_kernel(const unsigned long long* __restrict__ words, int64_t pixels,
                                                             int32_t* __restrict__ image1, int32_t* __restrict__ image2) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= 2 * pixels) return;
    const int32_t label = (int32_t)(words[e] & 0xFFull);
    int32_t* img = e < pixels ? image1 : image2;
    const int64_t k = e < pixels ? e : e - pixels;
    reinterpret_cast<int2*>(img)[k] = make_int2(0, label);  // channel 0 (instance id) stays 0
}

bool ri_args_ok(const void* pred, int32_t pred_bytes, const int32_t* ri, int64_t n, int32_t rows, int32_t cols,
                int32_t n_classes, const int32_t* image1, const int32_t* image2, const int32_t* n_outside) {
    if (n < 0 || rows < 1 || cols < 1 || (int64_t)rows * cols > (int64_t)1 << 28) return false;
    if (n_classes < 1 || n_classes > 254 || (pred_bytes != 1 && pred_bytes != 8)) return false;  // label + 1 in 8 bits
    if (n > 0 && (!pred || !ri)) return false;
    return image1 && image2 && n_outside;
}

}  // namespace

extern "C" {

int seg3d_frame_assemble(const seg3d_sweep_table* table, int32_t dim, int32_t point_bytes, void* out_rows,
                         float* out_f32, float* out_collated, float batch_id, void* stream) {
    SweepStarts st;
    if (!table_ok(table, dim, point_bytes, &st)) return SEG3D_EINVAL;
    const int64_t total = st.start[table->n_sweeps];
    if (total == 0) return SEG3D_OK;
    if (!out_rows && !out_f32 && !out_collated) return SEG3D_EINVAL;
    const int64_t tiles = ceil_div64(total, kTileRows);
    const unsigned nb = (unsigned)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
    if (point_bytes == 4)
        hipLaunchKernelGGL(frame_assemble_kernel<float>, dim3(nb), dim3(kThreads), 0, as_stream(stream), *table, st,
                           (int)dim, static_cast<float*>(out_rows), out_f32, out_collated, batch_id);
    else
        hipLaunchKernelGGL(frame_assemble_kernel<double>, dim3(nb), dim3(kThreads), 0, as_stream(stream), *table, st,
                           (int)dim, static_cast<double*>(out_rows), out_f32, out_collated, batch_id);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_frame_assemble_host(const seg3d_sweep_table* table, int32_t dim, int32_t point_bytes, void* out_rows,
                              float* out_f32, float* out_collated, float batch_id) {
    SweepStarts st;
    if (!table_ok(table, dim, point_bytes, &st)) return SEG3D_EINVAL;
    if (st.start[table->n_sweeps] == 0) return SEG3D_OK;
    if (!out_rows && !out_f32 && !out_collated) return SEG3D_EINVAL;
    if (point_bytes == 4)
        assemble_host<float>(*table, dim, static_cast<float*>(out_rows), out_f32, out_collated, batch_id);
    else
        assemble_host<double>(*table, dim, static_cast<double*>(out_rows), out_f32, out_collated, batch_id);
    return SEG3D_OK;
}

size_t seg3d_range_image_workspace_bytes(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1) return 0;
    return (size_t)2 * (size_t)rows * (size_t)cols * sizeof(unsigned long long);
}

int seg3d_range_image_labels(const void* pred, int32_t pred_bytes, const int32_t* points_ri, int64_t n, int32_t rows,
                             int32_t cols, int32_t n_classes, int32_t* image1, int32_t* image2, int32_t* n_outside,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!ri_args_ok(pred, pred_bytes, points_ri, n, rows, cols, n_classes, image1, image2, n_outside)) return SEG3D_EINVAL;
    const size_t need = seg3d_range_image_workspace_bytes(rows, cols);
    if (!workspace) return SEG3D_EINVAL;
    // the unpack pass stores (0, label) as one 8-byte word; the pixel words are 8 bytes
    if ((reinterpret_cast<uintptr_t>(image1) | reinterpret_cast<uintptr_t>(image2) | reinterpret_cast<uintptr_t>(workspace)) & 7)
        return SEG3D_EINVAL;
    if (workspace_bytes < need) return SEG3D_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const int64_t pixels = (int64_t)rows * cols;
    unsigned long long* words = static_cast<unsigned long long*>(workspace);
    SEG3D_CHECK_HIP(hipMemsetAsync(words, 0, need, st));
    SEG3D_CHECK_HIP(hipMemsetAsync(n_outside, 0, sizeof(int32_t), st));
    if (n > 0) {
        hipLaunchKernelGGL(ri_scatter_kernel, dim3((unsigned)ceil_div64(n, kThreads)), dim3(kThreads), 0, st, pred,
                           (int)pred_bytes, points_ri, n, (int)rows, (int)cols, (int)n_classes, words, n_outside);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ri_unpack_kernel, dim3((unsigned)ceil_div64(2 * pixels, kThreads)), dim3(kThreads), 0, st, words,
                       pixels, image1, image2);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_range_image_labels_host(const void* pred, int32_t pred_bytes, const int32_t* points_ri, int64_t n, int32_t rows,
                                  int32_t cols, int32_t n_classes, int32_t* image1, int32_t* image2, int32_t* n_outside) {
    if (!ri_args_ok(pred, pred_bytes, points_ri, n, rows, cols, n_classes, image1, image2, n_outside)) return SEG3D_EINVAL;
    const int64_t pixels = (int64_t)rows * cols;
    memset(image1, 0, (size_t)pixels * 2 * sizeof(int32_t));
    memset(image2, 0, (size_t)pixels * 2 * sizeof(int32_t));
    int32_t outside = 0;
    for (int64_t i = 0; i < n; ++i) {  // ascending: the highest index is the last writer
        const int64_t label = pred_at(pred, pred_bytes, i);
        int64_t pixel = 0;
        const int what = ri_target(points_ri + 3 * i, label, rows, cols, n_classes, &pixel);
        if (what == 1) {
            int32_t* img = pixel < pixels ? image1 : image2;
            img[2 * (pixel < pixels ? pixel : pixel - pixels) + 1] = (int32_t)(label + 1);
        } else if (what == 2) {
            ++outside;
        }
    }
    *n_outside = outside;
    return SEG3D_OK;
}

}  // extern "C"
