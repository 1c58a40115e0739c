// Per-point image features: the lookup loop of tools/extract_image_feature.py:84-100 -- for every lidar row, pick the
// first of its two camera projections whose camera has a feature map and copy that map's C values at (y, x).
//
// MI355X design.  Nothing is computed: the kernel moves 24-48 B of projection columns in and C floats out per row, and
// in between performs one dependent gather.  A workgroup owns 256 consecutive rows.
//   1. The six projection columns of the tile go into LDS with lane-consecutive element loads (a raw row is 60-120 B;
//      one row per lane would be a strided access), as csrc/frame.hip stages its rows.
//   2. One lane per row turns them into (camera, element offset of channel 0) with Python's int() and the reference's
//      if / elif, or into a miss.  The camera table (336 B, passed by value) sits in LDS because the camera is a per-lane
//      index.  Outside pixels are tallied per wave with a ballot; one lane adds the wave's count with an integer atomic.
//   3. The gather, in one of two lane assignments chosen per call:
//      channel-last (every present map has channel_stride 1: HWC): a row's C values are one contiguous segment, so
//      lanes run flat over (row, channel) -- loads are C-element segments, stores are lane-consecutive.
//      any other layout (CHW, sliced views): every channel of a pixel is a plane apart, so a lane keeps its row and
//      loops over the channels: the 64 loads of one wave-instruction are the same channel of 64 rows, which are
//      neighbouring pixels when the rows come in range-image order.  Up to 32 channels at a time are staged in LDS
//      (odd pitch: conflict-free stores) and streamed out lane-consecutively, so the [n, C] output is written in
//      contiguous spans whichever layout was read.
// All offsets are int64.  Nothing allocates or synchronises; no float arithmetic, so the host twin below (plain C++, no
// HIP call, the same decision function and the same half -> float conversion) gives the same bits.
#include <string.h>

#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 256;
constexpr int kMaxChannels = 64;
constexpr int kChunk = 32;           // channels staged at a time on the row-per-lane path
constexpr int kPitch = kChunk + 1;   // odd: lanes of one store hit 32 different banks
constexpr int kMaxBlocks = 1024;     // four workgroups per CU; larger inputs loop over tiles

// float16 bits -> float32, exact; a NaN comes out quiet with its payload, as the hardware conversion gives it
__host__ __device__ __forceinline__ float half_bits_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu, bits;
    if (exp == 0x1Fu) {
        bits = sign | 0x7F800000u | (man << 13) | (man ? 0x00400000u : 0u);
    } else if (exp != 0) {
        bits = sign | ((exp + 112u) << 23) | (man << 13);
    } else if (man == 0) {
        bits = sign;
    } else {  // subnormal: normalise
        int shift = 0;
        while (!(man & 0x400u)) {
            man <<= 1;
            ++shift;
        }
        bits = sign | ((uint32_t)(113 - shift) << 23) | ((man & 0x3FFu) << 13);
    }
    float f;
    memcpy(&f, &bits, sizeof(f));
    return f;
}

__host__ __device__ __forceinline__ float elem_to_float(float v) { return v; }
__host__ __device__ __forceinline__ float elem_to_float(uint16_t v) { return half_bits_to_float(v); }

// Python's int(v): truncation toward zero; false for a non-finite value or |v| >= 2^31
template <typename T>
__host__ __device__ __forceinline__ bool py_int(T v, int32_t* out) {
    if (!(v > (T)-2147483648.0 && v < (T)2147483648.0)) return false;
    *out = (int32_t)v;
    return true;
}

enum { kMiss = 0, kHit = 1, kOutside = 2 };

// extract_image_feature.py:90-97 on the six columns (name, x, y, name, x, y) of one row.  kHit: *camera and the element
// offset of channel 0.  kOutside: a column the decision read is not an int32, or the chosen camera's pixel is outside
// its map -- the second projection is NOT tried then, as the reference's elif is not.
template <typename T>
__host__ __device__ __forceinline__ int decide(const seg3d_feature_map* maps, int n_maps, const T* p, int32_t* camera,
                                               int64_t* offset) {
    for (int k = 0; k < 2; ++k, p += 3) {
        int32_t name;
        if (!py_int(p[0], &name)) return kOutside;
        const int64_t cam = (int64_t)name - 1;
        if (cam < 0 || cam >= n_maps || !maps[cam].data) continue;
        const seg3d_feature_map& m = maps[cam];
        int32_t x, y;
        if (!py_int(p[1], &x) || !py_int(p[2], &y)) return kOutside;
        if (x < 0 || x >= m.width || y < 0 || y >= m.height) return kOutside;
        *camera = (int32_t)cam;
        *offset = (int64_t)y * m.row_stride + (int64_t)x * m.col_stride;
        return kHit;
    }
    return kMiss;
}

template <typename T, typename E, bool kChannelLast>
__global__ __launch_bounds__(kThreads) void point_image_features_kernel(seg3d_feature_map_table tab,
                                                                        const T* __restrict__ rows, int64_t n, int stride,
                                                                        int cp_col, float* __restrict__ out_dense,
                                                                        int32_t* __restrict__ out_camera,
                                                                        int32_t* __restrict__ n_outside) {
    __shared__ seg3d_feature_map s_maps[SEG3D_IMAGE_MAX_CAMERAS];
    __shared__ __align__(16) float s_stage[kTileRows * kPitch];  // first the projection columns, then the staged channels
    __shared__ int64_t s_off[kTileRows];
    __shared__ int32_t s_cam[kTileRows];
    static_assert(sizeof(s_stage) >= sizeof(double) * 6 * kTileRows, "the projection columns share the stage");
    T* cols = reinterpret_cast<T*>(s_stage);
    const int t = threadIdx.x;
    const int C = tab.channels;
    if (t < SEG3D_IMAGE_MAX_CAMERAS) s_maps[t] = tab.maps[t];
    for (int64_t p0 = (int64_t)blockIdx.x * kTileRows; p0 < n; p0 += (int64_t)gridDim.x * kTileRows) {
        const int tile = (int)(n - p0 < kTileRows ? n - p0 : kTileRows);
        for (int e = t; e < tile * 6; e += kThreads) {
            const int r = e / 6, c = e - r * 6;
            cols[e] = rows[(p0 + r) * stride + cp_col + c];
        }
        __syncthreads();
        int32_t cam = -1;
        int64_t off = 0;
        int what = kMiss;
        if (t < tile) what = decide<T>(s_maps, tab.n_maps, cols + 6 * t, &cam, &off);
        if (what != kHit) cam = -1;
        const unsigned long long outside = __ballot(what == kOutside);
        if ((t & (SEG3D_WAVE - 1)) == 0 && outside) atomicAdd(n_outside, (int32_t)__popcll(outside));
        if (t < tile) out_camera[p0 + t] = cam;
        if (kChannelLast) {
            s_cam[t] = cam;
            s_off[t] = off;
            __syncthreads();
            float* dst = out_dense + p0 * C;
            for (int e = t; e < tile * C; e += kThreads) {
                const int r = e / C, c = e - r * C;
                const int32_t rc = s_cam[r];
                dst[e] = rc < 0 ? 0.0f : elem_to_float(static_cast<const E*>(s_maps[rc].data)[s_off[r] + c]);
            }
        } else {
            const E* src = cam < 0 ? nullptr : static_cast<const E*>(s_maps[cam].data) + off;
            const int64_t cs = cam < 0 ? 0 : s_maps[cam].channel_stride;
            for (int c0 = 0; c0 < C; c0 += kChunk) {
                const int cw = C - c0 < kChunk ? C - c0 : kChunk;
                __syncthreads();  // the columns, or the previous chunk, have been read
                if (t < tile) {
                    // every load of the chunk is issued before the first value is used (the loads are independent, each a
                    // different cache line); measured, it runs as fast as four loads in flight did
                    E v[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c)
                        v[c] = (src && c < cw) ? src[(int64_t)(c0 + c) * cs] : E(0);
#pragma unroll
                    for (int c = 0; c < kChunk; ++c)
                        if (c < cw) s_stage[t * kPitch + c] = elem_to_float(v[c]);
                }
                __syncthreads();
                for (int e = t; e < tile * cw; e += kThreads) {
                    const int r = e / cw, c = e - r * cw;
                    out_dense[(p0 + r) * C + c0 + c] = s_stage[r * kPitch + c];
                }
            }
        }
        __syncthreads();
    }
}

// SEG3D_EINVAL cases of the contract; nothing behind a pointer is read
bool args_ok(const seg3d_feature_map_table* tab, const void* rows, int32_t point_bytes, int64_t n, int32_t stride,
             int32_t cp_col, const float* out_dense, const int32_t* out_camera, const int32_t* n_outside) {
    if (!tab || tab->channels < 1 || tab->channels > kMaxChannels) return false;
    if (tab->n_maps < 1 || tab->n_maps > SEG3D_IMAGE_MAX_CAMERAS) return false;
    if ((tab->elem_bytes != 2 && tab->elem_bytes != 4) || (point_bytes != 4 && point_bytes != 8)) return false;
    if (cp_col < 0 || stride < 6 || cp_col > stride - 6) return false;
    if (n < 0 || n > (int64_t)INT32_MAX) return false;
    for (int m = 0; m < tab->n_maps; ++m) {
        const seg3d_feature_map& e = tab->maps[m];
        if (e.data && (e.height < 1 || e.width < 1 || e.channel_stride < 1 || e.row_stride < 1 || e.col_stride < 1))
            return false;
    }
    if (n > 0 && (!rows || !out_dense || !out_camera || !n_outside)) return false;
    return true;
}

bool channel_last(const seg3d_feature_map_table& tab) {
    for (int m = 0; m < tab.n_maps; ++m)
        if (tab.maps[m].data && tab.maps[m].channel_stride != 1) return false;
    return true;
}

template <typename T, typename E>
void launch(const seg3d_feature_map_table& tab, const void* rows, int64_t n, int stride, int cp_col, float* out_dense,
            int32_t* out_camera, int32_t* n_outside, hipStream_t st) {
    const int64_t tiles = ceil_div64(n, kTileRows);
    const dim3 grid((unsigned)(tiles < kMaxBlocks ? tiles : kMaxBlocks)), block(kThreads);
    if (channel_last(tab))
        hipLaunchKernelGGL((point_image_features_kernel<T, E, true>), grid, block, 0, st, tab, static_cast<const T*>(rows),
                           n, stride, cp_col, out_dense, out_camera, n_outside);
    else
        hipLaunchKernelGGL((point_image_features_kernel<T, E, false>), grid, block, 0, st, tab, static_cast<const T*>(rows),
                           n, stride, cp_col, out_dense, out_camera, n_outside);
}

template <typename T, typename E>
int32_t lookup_host(const seg3d_feature_map_table& tab, const T* rows, int64_t n, int64_t stride, int cp_col,
                    float* out_dense, int32_t* out_camera) {
    int32_t outside = 0;
    const int C = tab.channels;
    for (int64_t i = 0; i < n; ++i) {
        int32_t cam = -1;
        int64_t off = 0;
        const int what = decide<T>(tab.maps, tab.n_maps, rows + i * stride + cp_col, &cam, &off);
        float* dst = out_dense + i * C;
        if (what == kHit) {
            const E* src = static_cast<const E*>(tab.maps[cam].data) + off;
            const int64_t cs = tab.maps[cam].channel_stride;
            for (int c = 0; c < C; ++c) dst[c] = elem_to_float(src[(int64_t)c * cs]);
        } else {
            cam = -1;
            for (int c = 0; c < C; ++c) dst[c] = 0.0f;
            if (what == kOutside) ++outside;
        }
        out_camera[i] = cam;
    }
    return outside;
}

}  // namespace

extern "C" {

int seg3d_point_image_features(const seg3d_feature_map_table* table, const void* rows, int32_t point_bytes, int64_t n,
                               int32_t stride, int32_t cp_col, float* out_dense, int32_t* out_camera, int32_t* n_outside,
                               void* stream) {
    if (!args_ok(table, rows, point_bytes, n, stride, cp_col, out_dense, out_camera, n_outside)) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    hipStream_t st = as_stream(stream);
    SEG3D_CHECK_HIP(hipMemsetAsync(n_outside, 0, sizeof(int32_t), st));
    if (point_bytes == 4) {
        if (table->elem_bytes == 4)
            launch<float, float>(*table, rows, n, stride, cp_col, out_dense, out_camera, n_outside, st);
        else
            launch<float, uint16_t>(*table, rows, n, stride, cp_col, out_dense, out_camera, n_outside, st);
    } else {
        if (table->elem_bytes == 4)
            launch<double, float>(*table, rows, n, stride, cp_col, out_dense, out_camera, n_outside, st);
        else
            launch<double, uint16_t>(*table, rows, n, stride, cp_col, out_dense, out_camera, n_outside, st);
    }
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_point_image_features_host(const seg3d_feature_map_table* table, const void* rows, int32_t point_bytes, int64_t n,
                                    int32_t stride, int32_t cp_col, float* out_dense, int32_t* out_camera,
                                    int32_t* n_outside) {
    if (!args_ok(table, rows, point_bytes, n, stride, cp_col, out_dense, out_camera, n_outside)) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    int32_t outside;
    if (point_bytes == 4)
        outside = table->elem_bytes == 4
                      ? lookup_host<float, float>(*table, static_cast<const float*>(rows), n, stride, cp_col, out_dense, out_camera)
                      : lookup_host<float, uint16_t>(*table, static_cast<const float*>(rows), n, stride, cp_col, out_dense, out_camera);
    else
        outside = table->elem_bytes == 4
                      ? lookup_host<double, float>(*table, static_cast<const double*>(rows), n, stride, cp_col, out_dense, out_camera)
                      : lookup_host<double, uint16_t>(*table, static_cast<const double*>(rows), n, stride, cp_col, out_dense, out_camera);
    *n_outside = outside;
    return SEG3D_OK;
}

}  // extern "C"
