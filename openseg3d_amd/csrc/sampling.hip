// sampling_ext: furthest-point sampling over batch segments, and the two small kernels of the sectorized variant.
// Reference: seg3d/ops/sampling/src/sampling_cuda.cu:19-134 (one block per segment, tmp[] in global memory, an
// eleven-barrier shared-memory tree per pick), wrappers seg3d/ops/sampling/sampling.py:7-86.
//
// Semantics, per segment i with rows offset[i-1]:offset[i] and output slots new_offset[i-1]:new_offset[i]:
//   * the first pick is the segment's first row;
//   * every further pick is the row with the largest tmp[k] = fminf(tmp[k], d(k, last pick)), tmp starting at 1e10,
//     d = ((x2-x1)*(x2-x1) + (y2-y1)*(y2-y1)) + (z2-z1)*(z2-z1) in float32, every operation rounded (no FMA
//     contraction, the convention of knn.hip; the library is built with -ffp-contract=off, host code included);
//   * ties go to the lowest row of the segment (the reference's winner among exactly equal distances is an artefact of
//     its reduction tree and changes with the block size); without exact ties both rules pick the same rows;
//   * a segment with 0 slots writes nothing; a segment with 0 rows and slots gets -1 in its slots; a segment asked for
//     more picks than it has rows keeps producing its lowest row of distance 0;
//   * with `order`, row k of a segment is xyz[order[k]] and the value returned is order[k] ("lowest row" = lowest k).
//
// MI355X design: one workgroup of 1024 threads (16 waves) per segment, the picks are a serial chain.  Each workgroup
// chooses its tier from its own segment length.  Resident tier (<= 1024 * 16 rows): every thread keeps 16 rows
// (x, y, z, tmp) in registers for the whole loop.  Streaming tier: a prologue writes x, y, z and tmp = 1e10 as four planes
// into the workspace (16 bytes per row), the loop reads 16 bytes and writes 4 per row and pick.  The arg-max reduces the
// 64-bit key (bits(tmp) << 32) | (0xFFFFFFFF - row) with a plain unsigned max -- tmp is >= 0 and never NaN, so its bit
// pattern is monotone, and the low word implements the tie rule: six cross-lane steps per wave, 16 wave keys (with the
// winner's coordinates beside them) to one of two alternating LDS slot arrays, one barrier, and every wave reduces
// the 16 keys again for itself.  One barrier per pick.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / SEG3D_WAVE;
constexpr int kFpsP = 16;  // rows per thread of the resident tier
constexpr int kFpsResident = kFpsThreads * kFpsP;
constexpr float kFpsFar = 1e10f;

struct alignas(16) FpsSlot {
    u64 key;
    float x, y, z, pad;
};

// max with the lane a DPP pattern names (all lanes active, full row and bank masks)
template <int CTRL>
__device__ __forceinline__ u64 dpp_max(u64 v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    const u64 o = ((u64)(unsigned)hi << 32) | (unsigned)lo;
    return o > v ? o : v;
}

// every lane of a row of 16 lanes gets the row's maximum: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror 4, row_ror 8
__device__ __forceinline__ u64 row16_max(u64 v) {
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x124>(v);
    v = dpp_max<0x128>(v);
    return v;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
    v = row16_max(v);
    u64 o = __shfl_xor(v, 16);
    v = o > v ? o : v;
    o = __shfl_xor(v, 32);
    return o > v ? o : v;
}

__device__ __forceinline__ float dist2(float x2, float y2, float z2, float x1, float y1, float z1) {
    const float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
    return (dx * dx + dy * dy) + dz * dz;
}

struct FpsPick {
    int k;
    float x, y, z;
};

// block-wide arg-max of the per-thread candidates; one barrier.  slots = two arrays of kFpsWaves entries.
__device__ __forceinline__ FpsPick block_argmax(float best, int bk, float bx, float by, float bz, FpsSlot* slots, int buf) {
    const u64 key = ((u64)__float_as_uint(best) << 32) | (u64)(0xFFFFFFFFu - (unsigned)bk);
    const u64 wmax = wave_max(key);
    const int wave = threadIdx.x / SEG3D_WAVE, lane = threadIdx.x % SEG3D_WAVE;
    FpsSlot* s = slots + buf * kFpsWaves;
    if (key == wmax) {  // keys are unique: exactly one lane per wave
        s[wave].key = key;
        s[wave].x = bx;
        s[wave].y = by;
        s[wave].z = bz;
    }
    __syncthreads();
    const u64 bmax = row16_max(s[lane % kFpsWaves].key);
    FpsPick p;
    p.k = (int)(0xFFFFFFFFu - (unsigned)bmax);
    const FpsSlot* w = s + (p.k % kFpsThreads) / SEG3D_WAVE;  // row k belongs to thread k % 1024 in both tiers
    p.x = w->x;
    p.y = w->y;
    p.z = w->z;
    return p;
}

// The streaming tier's rows of one segment: four planes x, y, z, tmp, `plane` floats apart.  Planes, not 16-byte records:
// the 4-byte tmp store of a wave is then 256 contiguous bytes instead of 64 pieces spread over 1 KiB, which halved the
// time per pick.  The base is wave-uniform, the row a 32-bit offset.
__device__ __forceinline__ float4 rec_load(const float* seg, int64_t plane, int k) {
    return make_float4(seg[k], (seg + plane)[k], (seg + 2 * plane)[k], (seg + 3 * plane)[k]);
}
__device__ __forceinline__ void rec_store(float* seg, int64_t plane, int k, float4 r) {
    seg[k] = r.x;
    (seg + plane)[k] = r.y;
    (seg + 2 * plane)[k] = r.z;
    (seg + 3 * plane)[k] = r.w;
}

constexpr int kFpsU = 8;  // rows a thread of the streaming tier loads before it needs the first

__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ xyz, int n,
                                                          const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ offset,
                                                          const int32_t* __restrict__ new_offset, int32_t* idx,
                                                          float* __restrict__ records, int64_t plane) {
    __shared__ FpsSlot slots[2 * kFpsWaves];
    const int seg = blockIdx.x, t = threadIdx.x;
    int start_n = seg == 0 ? 0 : offset[seg - 1], end_n = offset[seg];
    const int start_m = seg == 0 ? 0 : new_offset[seg - 1], end_m = new_offset[seg];
    end_n = min(end_n, n);  // never read past the arrays whatever the offsets say
    start_n = max(start_n, 0);
    const int len = end_n - start_n, m = end_m - start_m;
    if (m <= 0 || start_m < 0) return;
    if (len <= 0) {
        for (int j = t; j < m; j += kFpsThreads) idx[start_m + j] = -1;
        return;
    }
    // position (row of the concatenated segments) -> row of xyz, -1 for an order entry outside [0, n)
    auto row_of = [&](int pos) -> int {
        const int g = order ? order[pos] : pos;
        return (unsigned)g < (unsigned)n ? g : -1;
    };
    float cx = 0.f, cy = 0.f, cz = 0.f;  // the last pick
    {
        const int g = row_of(start_n);
        if (g >= 0) {
            cx = xyz[3 * (int64_t)g];
            cy = xyz[3 * (int64_t)g + 1];
            cz = xyz[3 * (int64_t)g + 2];
        }
    }
    if (t == 0) idx[start_m] = start_n;

    if (len <= kFpsResident) {
        // rows t, t + 1024, ..; a slot past the segment holds tmp = 0 at a row number above every real row: fminf keeps
        // it at 0 and the key order puts it behind every real row, so it is never picked and needs no branch
        float x[kFpsP], y[kFpsP], z[kFpsP], tmp[kFpsP];
#pragma unroll
        for (int p = 0; p < kFpsP; ++p) {
            const int k = t + p * kFpsThreads;
            const int g = k < len ? row_of(start_n + k) : -1;
            x[p] = y[p] = z[p] = 0.f;
            tmp[p] = 0.f;
            if (g >= 0) {
                x[p] = xyz[3 * (int64_t)g];
                y[p] = xyz[3 * (int64_t)g + 1];
                z[p] = xyz[3 * (int64_t)g + 2];
                tmp[p] = kFpsFar;
            }
        }
        for (int j = 1; j < m; ++j) {
            float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
            int bk = t;
#pragma unroll
            for (int p = 0; p < kFpsP; ++p) {
                const float d = fminf(tmp[p], dist2(x[p], y[p], z[p], cx, cy, cz));
                tmp[p] = d;
                if (d > best) {  // strict: the lowest row among equal distances
                    best = d;
                    bk = t + p * kFpsThreads;
                    bx = x[p];
                    by = y[p];
                    bz = z[p];
                }
            }
            const FpsPick pk = block_argmax(best, bk, bx, by, bz, slots, j & 1);
            cx = pk.x;
            cy = pk.y;
            cz = pk.z;
            if (t == 0) idx[start_m + j] = start_n + pk.k;
        }
    } else {
        float* seg_rec = records + start_n;
        for (int k = t; k < len; k += kFpsThreads) {
            const int g = row_of(start_n + k);
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g >= 0) r = make_float4(xyz[3 * (int64_t)g], xyz[3 * (int64_t)g + 1], xyz[3 * (int64_t)g + 2], kFpsFar);
            rec_store(seg_rec, plane, k, r);  // read back by this thread only
        }
        for (int j = 1; j < m; ++j) {
            float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
            int bk = t;
            // kFpsU rows at a time: all loads are issued before the first distance is needed
            for (int k0 = t; k0 < len; k0 += kFpsU * kFpsThreads) {
                float4 r[kFpsU];
#pragma unroll
                for (int u = 0; u < kFpsU; ++u) {
                    const int k = k0 + u * kFpsThreads;
                    if (k < len) r[u] = rec_load(seg_rec, plane, k);
                }
#pragma unroll
                for (int u = 0; u < kFpsU; ++u) {
                    const int k = k0 + u * kFpsThreads;
                    if (k < len) {
                        const float d = fminf(r[u].w, dist2(r[u].x, r[u].y, r[u].z, cx, cy, cz));
                        (seg_rec + 3 * plane)[k] = d;
                        if (d > best) {
                            best = d;
                            bk = k;
                            bx = r[u].x;
                            by = r[u].y;
                            bz = r[u].z;
                        }
                    }
                }
            }
            const FpsPick pk = block_argmax(best, bk, bx, by, bz, slots, j & 1);
            cx = pk.x;
            cy = pk.y;
            cz = pk.z;
            if (t == 0) idx[start_m + j] = start_n + pk.k;
        }
    }
    if (order) {  // positions -> rows of xyz; the barrier orders thread 0's stores before the workgroup's loads
        __syncthreads();
        for (int j = t; j < m; j += kFpsThreads) idx[start_m + j] = order[idx[start_m + j]];
    }
}

// ------------------------------------------------------------------------------------------------ sector partition
constexpr int kThreads = 256;

// sampling.py:49 writes atan2(x, y), x first.  Evaluated in double and rounded once, like atan2_t of voxelize.hip.
__host__ __device__ inline float sector_angle(float x, float y) { return (float)atan2((double)x, (double)y); }

__global__ __launch_bounds__(kThreads) void sector_angle_kernel(const float* __restrict__ xyz, int n, float* __restrict__ angle) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) angle[i] = sector_angle(xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1]);
}

// one workgroup per sample: min and max of its angles; NaN if any angle is NaN (torch.min / torch.max) or there is no row
__global__ __launch_bounds__(kFpsThreads) void sector_minmax_kernel(const float* __restrict__ angle, int n,
                                                                    const int32_t* __restrict__ offset,
                                                                    float* __restrict__ minmax) {
    __shared__ float s_lo[kFpsWaves], s_hi[kFpsWaves];
    __shared__ int s_nan[kFpsWaves];
    const int b = blockIdx.x, t = threadIdx.x;
    const int start = max(b == 0 ? 0 : offset[b - 1], 0), end = min(offset[b], n);
    float lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    for (int i = start + t; i < end; i += kFpsThreads) {
        const float a = angle[i];
        nan |= a != a;
        lo = fminf(lo, a);
        hi = fmaxf(hi, a);
    }
    for (int s = 1; s < SEG3D_WAVE; s <<= 1) {
        lo = fminf(lo, __shfl_xor(lo, s));
        hi = fmaxf(hi, __shfl_xor(hi, s));
        nan |= __shfl_xor(nan, s);
    }
    if (t % SEG3D_WAVE == 0) {
        s_lo[t / SEG3D_WAVE] = lo;
        s_hi[t / SEG3D_WAVE] = hi;
        s_nan[t / SEG3D_WAVE] = nan;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kFpsWaves; ++w) {
            lo = fminf(lo, s_lo[w]);
            hi = fmaxf(hi, s_hi[w]);
            nan |= s_nan[w];
        }
        if (nan || end <= start) lo = hi = NAN;
        minmax[2 * b] = lo;
        minmax[2 * b + 1] = hi;
    }
}

// Both searches are linear: batch sizes and sector counts are in the tens (sampling.py's callers: a handful of samples,
// 8-16 sectors), where a bisection would save nothing.
// sector of a row: the first s of its sample with edge[s] <= a < edge[s+1] (sampling.py:53), global id = sectors of the
// samples before + s; -1 if there is none (NaN angles).  Sample b has sector_offset[b+1] - sector_offset[b] sectors and
// one edge more, its edges start at edges[sector_offset[b] + b].
__host__ __device__ inline int32_t sector_of(float a, int b, const float* edges, const int32_t* sector_offset) {
    const int s0 = sector_offset[b], ns = sector_offset[b + 1] - s0;
    const float* e = edges + s0 + b;
    for (int s = 0; s < ns; ++s)
        if (a >= e[s] && a < e[s + 1]) return s0 + s;
    return -1;
}

__global__ __launch_bounds__(kThreads) void sector_assign_kernel(const float* __restrict__ angle, int n,
                                                                 const int32_t* __restrict__ offset, int batch,
                                                                 const float* __restrict__ edges,
                                                                 const int32_t* __restrict__ sector_offset,
                                                                 int32_t* __restrict__ sector_id) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    int b = 0;
    while (b < batch && i >= offset[b]) ++b;
    sector_id[i] = b < batch ? sector_of(angle[i], b, edges, sector_offset) : -1;
}

bool fps_args_ok(int64_t n, int32_t n_segments) { return n >= 0 && n < (int64_t)0x7FFFFFF0 && n_segments >= 0; }

}  // namespace

extern "C" size_t seg3d_furthest_sampling_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (int64_t)0x7FFFFFF0) return 0;
    return 16 * align_up((size_t)n, 64) + 256;
}

extern "C" int seg3d_furthest_sampling(const float* xyz, int64_t n, const int32_t* order, const int32_t* offset,
                                       const int32_t* new_offset, int32_t n_segments, int32_t* idx, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!fps_args_ok(n, n_segments)) return SEG3D_EINVAL;
    if (n_segments == 0) return SEG3D_OK;
    if (!offset || !new_offset || !idx || (n > 0 && !xyz)) return SEG3D_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < seg3d_furthest_sampling_workspace_bytes(n))
        return SEG3D_EWORKSPACE;
    hipLaunchKernelGGL(fps_kernel, dim3((unsigned)n_segments), dim3(kFpsThreads), 0, as_stream(stream), xyz, (int)n, order,
                       offset, new_offset, idx, static_cast<float*>(workspace), (int64_t)align_up((size_t)n, 64));
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

// The host twin: the same arithmetic and tie rule in plain serial C++, no HIP call.
extern "C" int seg3d_furthest_sampling_host(const float* xyz, int64_t n, const int32_t* order, const int32_t* offset,
                                            const int32_t* new_offset, int32_t n_segments, int32_t* idx) {
    if (!fps_args_ok(n, n_segments)) return SEG3D_EINVAL;
    if (n_segments == 0) return SEG3D_OK;
    if (!offset || !new_offset || !idx || (n > 0 && !xyz)) return SEG3D_EINVAL;
    std::vector<float> px, py, pz, tmp;
    std::vector<int32_t> row;
    for (int seg = 0; seg < n_segments; ++seg) {
        int64_t start_n = seg == 0 ? 0 : offset[seg - 1], end_n = offset[seg];
        const int64_t start_m = seg == 0 ? 0 : new_offset[seg - 1], end_m = new_offset[seg];
        if (end_n > n) end_n = n;
        if (start_n < 0) start_n = 0;
        const int64_t len = end_n - start_n, m = end_m - start_m;
        if (m <= 0 || start_m < 0) continue;
        if (len <= 0) {
            for (int64_t j = 0; j < m; ++j) idx[start_m + j] = -1;
            continue;
        }
        px.assign((size_t)len, 0.f);
        py.assign((size_t)len, 0.f);
        pz.assign((size_t)len, 0.f);
        tmp.assign((size_t)len, 0.f);
        row.assign((size_t)len, 0);
        for (int64_t k = 0; k < len; ++k) {
            const int32_t g = order ? order[start_n + k] : (int32_t)(start_n + k);
            row[k] = g;
            if (g >= 0 && g < n) {
                px[k] = xyz[3 * (int64_t)g];
                py[k] = xyz[3 * (int64_t)g + 1];
                pz[k] = xyz[3 * (int64_t)g + 2];
                tmp[k] = kFpsFar;
            }
        }
        int64_t last = 0;
        idx[start_m] = row[0];
        for (int64_t j = 1; j < m; ++j) {
            const float cx = px[last], cy = py[last], cz = pz[last];
            float best = -1.f;
            int64_t bk = 0;
            for (int64_t k = 0; k < len; ++k) {
                const float dx = px[k] - cx, dy = py[k] - cy, dz = pz[k] - cz;
                const float d = fminf(tmp[k], (dx * dx + dy * dy) + dz * dz);
                tmp[k] = d;
                if (d > best) {
                    best = d;
                    bk = k;
                }
            }
            last = bk;
            idx[start_m + j] = row[bk];
        }
    }
    return SEG3D_OK;
}

extern "C" int seg3d_sector_angles(const float* xyz, int64_t n, const int32_t* offset, int32_t batch_size, float* angle,
                                   float* minmax, void* stream) {
    if (!fps_args_ok(n, batch_size)) return SEG3D_EINVAL;
    if (batch_size == 0) return SEG3D_OK;
    if (!offset || !minmax || (n > 0 && (!xyz || !angle))) return SEG3D_EINVAL;
    hipStream_t st = as_stream(stream);
    if (n > 0) {
        hipLaunchKernelGGL(sector_angle_kernel, dim3((unsigned)ceil_div64(n, kThreads)), dim3(kThreads), 0, st, xyz, (int)n,
                           angle);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sector_minmax_kernel, dim3((unsigned)batch_size), dim3(kFpsThreads), 0, st, angle, (int)n, offset, minmax);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_sector_angles_host(const float* xyz, int64_t n, const int32_t* offset, int32_t batch_size, float* angle,
                                        float* minmax) {
    if (!fps_args_ok(n, batch_size)) return SEG3D_EINVAL;
    if (batch_size == 0) return SEG3D_OK;
    if (!offset || !minmax || (n > 0 && (!xyz || !angle))) return SEG3D_EINVAL;
    for (int64_t i = 0; i < n; ++i) angle[i] = sector_angle(xyz[3 * i], xyz[3 * i + 1]);
    for (int b = 0; b < batch_size; ++b) {
        int64_t start = b == 0 ? 0 : offset[b - 1], end = offset[b];
        if (start < 0) start = 0;
        if (end > n) end = n;
        float lo = INFINITY, hi = -INFINITY;
        bool nan = end <= start;
        for (int64_t i = start; i < end; ++i) {
            const float a = angle[i];
            nan = nan || a != a;
            lo = fminf(lo, a);
            hi = fmaxf(hi, a);
        }
        minmax[2 * b] = nan ? NAN : lo;
        minmax[2 * b + 1] = nan ? NAN : hi;
    }
    return SEG3D_OK;
}

extern "C" int seg3d_sector_assign(const float* angle, int64_t n, const int32_t* offset, int32_t batch_size,
                                   const float* edges, const int32_t* sector_offset, int32_t* sector_id, void* stream) {
    if (!fps_args_ok(n, batch_size)) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    if (batch_size == 0 || !angle || !offset || !edges || !sector_offset || !sector_id) return SEG3D_EINVAL;
    hipLaunchKernelGGL(sector_assign_kernel, dim3((unsigned)ceil_div64(n, kThreads)), dim3(kThreads), 0, as_stream(stream), angle,
                       (int)n, offset, (int)batch_size, edges, sector_offset, sector_id);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_sector_assign_host(const float* angle, int64_t n, const int32_t* offset, int32_t batch_size,
                                        const float* edges, const int32_t* sector_offset, int32_t* sector_id) {
    if (!fps_args_ok(n, batch_size)) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    if (batch_size == 0 || !angle || !offset || !edges || !sector_offset || !sector_id) return SEG3D_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        int b = 0;
        while (b < batch_size && i >= offset[b]) ++b;
        sector_id[i] = b < batch_size ? sector_of(angle[i], b, edges, sector_offset) : -1;
    }
    return SEG3D_OK;
}
