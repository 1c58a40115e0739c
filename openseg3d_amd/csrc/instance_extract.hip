// Instance bank extraction on the device: DBSCAN over the xy of every target label's rows, then centre, radius and
// height above the nearest ground row of each cluster.
// Reference: tools/extract_instances.py:46-76 (one target label per run of the script, sklearn's DBSCAN, a Python loop
// over every point for the ground rows); include/seg3d_hip.h states the DBSCAN rule that is implemented.
//
// MI355X design: one call per frame, all target labels at once, a fixed chain of launches and no read-back.
//   keys     per row: label position (slot), cell = floor(xy / side) -> one 64-bit key slot | cx | cy (non-target: all ones)
//   sort     rocPRIM radix sort of (key, row): a cell is a run of the sorted keys, the three cells (cx', cy-1 .. cy+1) are
//            ONE contiguous key range, so the 3 x 3 block of a row is three ranges found by bisection -- no table
//   core     one lane per sorted row counts its neighbours (stops at min_points)
//   unite    lock-free union-find over the core rows: compare-and-swap that hooks the LARGER root under the smaller, so
//            parent[x] <= x always, every find walks strictly downward and the final root is the lowest core row
//   label    core rows take their root, border rows the lowest root among their core neighbours (= the lowest-numbered
//            cluster, since clusters of a label are numbered by root row); writes key (slot, root) per row
//   sort     stable radix sort of ((slot, root), row): cluster_rows in its final order; run heads + the exclusive scan of
//            scan.hip give the cluster numbers
//   stats    one workgroup per cluster: the fixed-order mean of augment_instance.hip, then the radius
//   ground   one sweep over the frame per eight clusters: per cluster the lexicographic minimum (d, row) over the ground
//            rows, wave64 shuffles -> LDS -> one record per workgroup; a fold decides kept / height
// Counts are integers, minima are exact and the sums have one order: the result is a pure function of the inputs.  The
// host twin below shares every recipe (the key, the bisection, the distance tests) and gives the same bits.
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "instance_geom.hpp"

// fixed sequences of IEEE products and sums, as numpy rounds them; no fused multiply-add (see augment.hip)
#pragma clang fp contract(off)

namespace {

constexpr int kWaves = kThreads / SEG3D_WAVE;
constexpr int kMaxDim = 16;
constexpr int kMaxTargets = 8;
constexpr int kMaxGround = 8;
constexpr int kChunk = 8;              // clusters one ground workgroup carries in registers
constexpr int kMaxGroundBlocks = 64;   // row blocks of the ground sweep: 16 384 lanes, eleven rows each at 175 k
constexpr int kMaxStatBlocks = 1024;
constexpr int32_t kMaxCap = 1 << 18;  // the ground sweep's grid.y is cap / 8
constexpr int32_t kNoRow = INT32_MAX;
constexpr int kCellBits = 29;
constexpr double kCellHalf = 268435456.0;  // 2^28: cells are clamped to [-2^28, 2^28)
constexpr unsigned kCellKeyBits = 4 + 2 * kCellBits;  // bit 61 is set only in kNoKey: non-target rows sort behind every cell
constexpr unsigned kRootKeyBits = 3 + 32;
constexpr uint64_t kNoKey = ~0ull;

struct ExtractParams {
    uint8_t slot_of[256];  // position of a label in target_ids, 0xFF: not a target
    uint8_t is_ground[256];
    int32_t min_points[kMaxTargets];
    int32_t label_of[kMaxTargets];
    double eps2;
    double side;  // cell side: eps * (1 + 2^-20), see cell_of
};

struct GroundRec {
    double d;
    int32_t row;
    int32_t pad;
};

// Cell of a coordinate, shifted to [0, 2^29).  Two rows within eps of each other must land in the same or in adjacent
// cells although v / side is rounded: with side = eps * (1 + 2^-20) their exact quotients differ by less than
// 1 - 2^-21, and the two roundings move them by at most 2^-24 each while |cell| < 2^28.  Beyond that the clamp puts
// everything into one cell, which only adds candidates; the neighbour test itself is exact.  NaN goes to cell 0.
__host__ __device__ __forceinline__ uint64_t cell_of(double v, double side) {
    double c = floor(v / side);
    if (!(c >= -kCellHalf)) c = -kCellHalf;
    if (c > kCellHalf - 1.0) c = kCellHalf - 1.0;
    return (uint64_t)((int64_t)c + (int64_t)kCellHalf);
}

__host__ __device__ __forceinline__ uint64_t make_key(uint64_t slot, uint64_t cx, uint64_t cy) {
    return (slot << (2 * kCellBits)) | (cx << kCellBits) | cy;
}

// first position in keys [0, n) that is >= key
__host__ __device__ __forceinline__ int64_t lower_bound_key(const uint64_t* __restrict__ keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// f(row j) for every row of the 3 x 3 cells around the row with `key` at (x, y) that is its neighbour (itself included),
// in no particular order; f returns false to stop
template <typename T, typename F>
__host__ __device__ __forceinline__ void for_each_neighbour(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ srows,
                                                            int64_t n, const T* __restrict__ pts, int dim, uint64_t key, double x,
                                                            double y, double eps2, F&& f) {
    const uint64_t cmask = (1ull << kCellBits) - 1;
    const uint64_t slot = key >> (2 * kCellBits), cx = (key >> kCellBits) & cmask, cy = key & cmask;
    const uint64_t y0 = cy > 0 ? cy - 1 : 0, y1 = cy < cmask ? cy + 1 : cmask;
    for (int ox = -1; ox <= 1; ++ox) {
        if ((ox < 0 && cx == 0) || (ox > 0 && cx == cmask)) continue;
        const uint64_t nx = cx + ox;
        int64_t q = lower_bound_key(skeys, n, make_key(slot, nx, y0));
        const uint64_t last = make_key(slot, nx, y1);
        for (; q < n && skeys[q] <= last; ++q) {
            const int64_t j = srows[q];
            const double dx = x - (double)pts[j * dim], dy = y - (double)pts[j * dim + 1];
            if (dx * dx + dy * dy <= eps2)
                if (!f((int32_t)j)) return;
        }
    }
}

// label_at, closer and dist3 (np.linalg.norm, :29-31, :69) are instance_geom.hpp's, shared with augment_instance.hip

// ------------------------------------------------------------------------------------------ device
// the running counters are the caller's counts[4], zeroed by a memset in front of the chain
template <typename T>
__global__ __launch_bounds__(kThreads) void ext_keys_kernel(const T* __restrict__ pts, int64_t n, int dim,
                                                            const void* __restrict__ labels, int label_bytes, ExtractParams P,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ rows,
                                                            uint64_t* __restrict__ root_keys, uint32_t* __restrict__ root_rows,
                                                            int32_t* __restrict__ parent, int32_t* __restrict__ point_cluster,
                                                            int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t l = label_at(labels, label_bytes, i);
    const uint32_t slot = (l >= 0 && l < 256) ? P.slot_of[l] : 0xFFu;
    uint64_t key = kNoKey;
    if (slot != 0xFFu) {
        key = make_key(slot, cell_of((double)pts[i * dim], P.side), cell_of((double)pts[i * dim + 1], P.side));
        atomicAdd(&counts[3], 1);
    }
    keys[i] = key;
    rows[i] = (uint32_t)i;
    root_keys[i] = kNoKey;
    root_rows[i] = (uint32_t)i;
    parent[i] = -1;
    point_cluster[i] = -1;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ext_core_kernel(const T* __restrict__ pts, int64_t n, int dim, ExtractParams P,
                                                            const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ srows,
                                                            int32_t* __restrict__ parent) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const uint64_t key = skeys[q];
    if (key == kNoKey) return;
    const int64_t i = srows[q];
    const int need = P.min_points[key >> (2 * kCellBits)];
    int cnt = 0;
    for_each_neighbour(skeys, srows, n, pts, dim, key, (double)pts[i * dim], (double)pts[i * dim + 1], P.eps2, [&](int32_t) {
        return ++cnt < need;
    });
    if (cnt >= need) parent[i] = (int32_t)i;
}

// walks strictly downward: parent[x] <= x at all times, a root has parent[x] == x
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
        if (p == x) return x;
        x = p;
    }
}

// A failed compare-and-swap means another lane has hooked `a` meanwhile, under something smaller: the retry starts from
// a strictly smaller pair of roots, so the loop ends without waiting for anybody.
__device__ __forceinline__ void uf_unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(&parent[a], a, b) == a) return;
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ext_unite_kernel(const T* __restrict__ pts, int64_t n, int dim, ExtractParams P,
                                                             const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ srows,
                                                             int32_t* __restrict__ parent) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const uint64_t key = skeys[q];
    if (key == kNoKey) return;
    const int32_t i = (int32_t)srows[q];
    if (__atomic_load_n(&parent[i], __ATOMIC_RELAXED) < 0) return;  // not core: the flags are final since ext_core_kernel
    for_each_neighbour(skeys, srows, n, pts, dim, key, (double)pts[(int64_t)i * dim], (double)pts[(int64_t)i * dim + 1], P.eps2,
                       [&](int32_t j) {
                           if (j < i && __atomic_load_n(&parent[j], __ATOMIC_RELAXED) >= 0) uf_unite(parent, i, j);
                           return true;
                       });
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ext_label_kernel(const T* __restrict__ pts, int64_t n, int dim, ExtractParams P,
                                                             const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ srows,
                                                             int32_t* __restrict__ parent, uint64_t* __restrict__ root_keys) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const uint64_t key = skeys[q];
    if (key == kNoKey) return;
    const int32_t i = (int32_t)srows[q];
    int32_t root = kNoRow;
    if (parent[i] >= 0) {
        root = uf_find(parent, i);
    } else {
        for_each_neighbour(skeys, srows, n, pts, dim, key, (double)pts[(int64_t)i * dim], (double)pts[(int64_t)i * dim + 1],
                           P.eps2, [&](int32_t j) {
                               if (parent[j] >= 0) {
                                   const int32_t r = uf_find(parent, j);
                                   root = r < root ? r : root;
                               }
                               return true;
                           });
    }
    if (root != kNoRow) root_keys[i] = ((key >> (2 * kCellBits)) << 32) | (uint64_t)(uint32_t)root;
}

// after the stable sort by (slot, root): run heads, and the number of clustered rows
__global__ __launch_bounds__(kThreads) void ext_heads_kernel(const uint64_t* __restrict__ rkeys, int64_t n,
                                                             uint32_t* __restrict__ flags, int32_t* __restrict__ counts) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const uint64_t key = rkeys[q];
    flags[q] = (key != kNoKey && (q == 0 || rkeys[q - 1] != key)) ? 1u : 0u;
    if (key != kNoKey && (q == n - 1 || rkeys[q + 1] == kNoKey)) counts[2] = (int32_t)(q + 1);
}

__global__ __launch_bounds__(kThreads) void ext_emit_kernel(const uint64_t* __restrict__ rkeys, const uint32_t* __restrict__ rrows,
                                                            int64_t n, const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ excl, int32_t cap,
                                                            int32_t* __restrict__ point_cluster, int32_t* __restrict__ cluster_rows,
                                                            int32_t* __restrict__ cbegin) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const uint64_t key = rkeys[q];
    if (key == kNoKey) {
        cluster_rows[q] = -1;
        return;
    }
    const int32_t row = (int32_t)rrows[q];
    const int32_t c = (int32_t)(excl[q] + flags[q]) - 1;
    cluster_rows[q] = row;
    point_cluster[row] = c;
    if (flags[q] && c <= cap) cbegin[c] = (int32_t)q;  // cbegin has cap + 1 entries
}

// centre and radius of every cluster, the mean in the one order of block_sum3 (instance_geom.hpp)
template <typename T>
__global__ __launch_bounds__(kThreads) void ext_stats_kernel(const T* __restrict__ pts, int dim, ExtractParams P,
                                                             const uint64_t* __restrict__ rkeys,
                                                             const int32_t* __restrict__ cluster_rows,
                                                             const int32_t* __restrict__ cbegin, const int32_t* __restrict__ counts,
                                                             int32_t cap, seg3d_instance_cluster* __restrict__ clusters) {
    __shared__ double lds[3 * kThreads];
    const int t = threadIdx.x;
    const int32_t found = counts[0], used = found < cap ? found : cap;
    for (int32_t c = blockIdx.x; c < used; c += gridDim.x) {  // uniform per workgroup
        const int32_t begin = cbegin[c], end = c + 1 < found ? cbegin[c + 1] : counts[2];
        const int32_t m = end - begin;
        double ctr[3] = {0.0, 0.0, 0.0};
        for (int j = t; j < m; j += kThreads) {
            const T* row = pts + (int64_t)cluster_rows[begin + j] * dim;
            for (int a = 0; a < 3; ++a) ctr[a] += (double)row[a];
        }
        block_sum3(ctr, lds);
        for (int a = 0; a < 3; ++a) ctr[a] /= (double)m;
        double r = 0.0;
        for (int j = t; j < m; j += kThreads) {
            const T* row = pts + (int64_t)cluster_rows[begin + j] * dim;
            const double d = dist3((double)row[0], (double)row[1], (double)row[2], ctr);
            if (d > r) r = d;
        }
        r = block_max(r, lds);
        if (t == 0) {
            seg3d_instance_cluster o;
            o.label = P.label_of[rkeys[begin] >> 32];
            o.begin = begin;
            o.rows = m;
            o.kept = 0;
            o.center[0] = ctr[0];
            o.center[1] = ctr[1];
            o.center[2] = ctr[2];
            o.radius = r;
            o.height = 0.0;
            clusters[c] = o;
        }
        __syncthreads();
    }
}

// every row of the frame once per chunk of eight clusters; workgroup (bx, chunk) leaves recs[bx * cap + c]
template <typename T>
__global__ __launch_bounds__(kThreads) void ext_ground_kernel(const T* __restrict__ pts, int64_t n, int dim,
                                                              const void* __restrict__ labels, int label_bytes, ExtractParams P,
                                                              const int32_t* __restrict__ counts, int32_t cap,
                                                              const seg3d_instance_cluster* __restrict__ clusters,
                                                              GroundRec* __restrict__ recs) {
    __shared__ double s_d[kWaves][kChunk];
    __shared__ int32_t s_row[kWaves][kChunk];
    const int t = threadIdx.x;
    const int32_t found = counts[0], used = found < cap ? found : cap;
    const int32_t c0 = (int32_t)blockIdx.y * kChunk;
    if (c0 >= used) return;  // uniform per workgroup
    double ctr[kChunk][3], bd[kChunk];
    int32_t brow[kChunk];
#pragma unroll
    for (int c = 0; c < kChunk; ++c) {
        const bool on = c0 + c < used;
        for (int a = 0; a < 3; ++a) ctr[c][a] = on ? clusters[c0 + c].center[a] : 0.0;
        bd[c] = INFINITY;
        brow[c] = kNoRow;
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + t; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t l = label_at(labels, label_bytes, i);
        if (l < 0 || l > 255 || !P.is_ground[l]) continue;
        const double x = (double)pts[i * dim], y = (double)pts[i * dim + 1], z = (double)pts[i * dim + 2];
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const double d = dist3(x, y, z, ctr[c]);
            if (closer(d, (int32_t)i, bd[c], brow[c])) {
                bd[c] = d;
                brow[c] = (int32_t)i;
            }
        }
    }
    // wave64: xor butterflies; the lexicographic minimum is exact, so the order does not show in the result
    for (int off = SEG3D_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const double od = __shfl_xor(bd[c], off, SEG3D_WAVE);
            const int32_t orow = __shfl_xor(brow[c], off, SEG3D_WAVE);
            if (closer(od, orow, bd[c], brow[c])) {
                bd[c] = od;
                brow[c] = orow;
            }
        }
    }
    const int wave = t / SEG3D_WAVE;
    if (t % SEG3D_WAVE == 0) {
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            s_d[wave][c] = bd[c];
            s_row[wave][c] = brow[c];
        }
    }
    __syncthreads();
    if (t < kChunk && c0 + t < used) {
        GroundRec r = {s_d[0][t], s_row[0][t], 0};
        for (int w = 1; w < kWaves; ++w)
            if (closer(s_d[w][t], s_row[w][t], r.d, r.row)) {
                r.d = s_d[w][t];
                r.row = s_row[w][t];
            }
        recs[(int64_t)blockIdx.x * cap + c0 + t] = r;
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ext_fold_kernel(const T* __restrict__ pts, int dim, int32_t* __restrict__ counts,
                                                            int32_t cap, int nb, const GroundRec* __restrict__ recs,
                                                            seg3d_instance_cluster* __restrict__ clusters) {
    const int32_t found = counts[0], used = found < cap ? found : cap;
    const int32_t c = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (c >= used) return;
    GroundRec best = {INFINITY, kNoRow, 0};
    for (int b = 0; b < nb; ++b) {
        const GroundRec r = recs[(int64_t)b * cap + c];
        if (closer(r.d, r.row, best.d, best.row)) best = r;
    }
    if (best.row != kNoRow && best.d < 1.2 * clusters[c].radius) {
        clusters[c].kept = 1;
        clusters[c].height = clusters[c].center[2] - (double)pts[(int64_t)best.row * dim + 2];
        atomicAdd(&counts[1], 1);
    }
}

struct ExtWs {
    uint64_t* keys[4];  // [n] each: cell keys (double-buffered), then (slot, root) keys (double-buffered)
    uint32_t* rows[4];
    int32_t* parent;    // [n]
    uint32_t* flags;    // [n]
    uint32_t* excl;     // [n]
    uint32_t* scan_tmp;
    int32_t* cbegin;    // [cap + 1]
    GroundRec* recs;    // [kMaxGroundBlocks * cap]
    void* sort_tmp;
    size_t sort_tmp_bytes;
};

bool ext_sort_bytes(int64_t n, size_t* bytes) {
    *bytes = 0;
    if (n == 0) return true;
    rocprim::double_buffer<uint64_t> k(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
    size_t a = 0, b = 0;
    if (rocprim::radix_sort_pairs(nullptr, a, k, v, (size_t)n, 0u, kCellKeyBits) != hipSuccess) return false;
    if (rocprim::radix_sort_pairs(nullptr, b, k, v, (size_t)n, 0u, kRootKeyBits) != hipSuccess) return false;
    *bytes = a > b ? a : b;
    return true;
}

bool ext_carve(void* ws, int64_t n, int32_t cap, ExtWs* w, size_t* bytes) {
    if (!ext_sort_bytes(n, &w->sort_tmp_bytes)) return false;
    WsCarver c(ws);
    for (int i = 0; i < 4; ++i) w->keys[i] = c.take<uint64_t>((size_t)n + 1);
    for (int i = 0; i < 4; ++i) w->rows[i] = c.take<uint32_t>((size_t)n + 1);
    w->parent = c.take<int32_t>((size_t)n + 1);
    w->flags = c.take<uint32_t>((size_t)n + 1);
    w->excl = c.take<uint32_t>((size_t)n + 1);
    w->scan_tmp = c.take<uint32_t>(scan_tmp_count(n));
    w->cbegin = c.take<int32_t>((size_t)cap + 1);
    w->recs = c.take<GroundRec>((size_t)kMaxGroundBlocks * (size_t)(cap > 0 ? cap : 1));
    w->sort_tmp = c.take<char>(w->sort_tmp_bytes + 1);
    if (bytes) *bytes = c.off;
    return true;
}

bool ext_args_ok(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels, int32_t label_bytes,
                 const uint8_t* target_ids, const int32_t* min_points, int32_t k, const uint8_t* ground_ids, int32_t g, double eps,
                 int32_t cap, const int32_t* point_cluster, const int32_t* cluster_rows, const seg3d_instance_cluster* clusters,
                 const int32_t* counts, ExtractParams* P) {
    if (n < 0 || n > INT32_MAX - 1 || dim < 3 || dim > kMaxDim || (point_bytes != 4 && point_bytes != 8)) return false;
    if ((label_bytes != 1 && label_bytes != 8) || k < 1 || k > kMaxTargets || g < 1 || g > kMaxGround) return false;
    if (!target_ids || !min_points || !ground_ids || !(eps > 0.0) || !(eps < INFINITY) || cap < 0 || cap > kMaxCap || !counts) return false;
    if (n > 0 && (!points || !labels || !point_cluster || !cluster_rows)) return false;
    if (cap > 0 && !clusters) return false;
    memset(P->slot_of, 0xFF, sizeof(P->slot_of));
    memset(P->is_ground, 0, sizeof(P->is_ground));
    for (int s = 0; s < kMaxTargets; ++s) P->min_points[s] = 1, P->label_of[s] = 0;
    for (int s = 0; s < k; ++s) {
        if (min_points[s] < 1 || P->slot_of[target_ids[s]] != 0xFF) return false;
        P->slot_of[target_ids[s]] = (uint8_t)s;
        P->min_points[s] = min_points[s];
        P->label_of[s] = target_ids[s];
    }
    for (int i = 0; i < g; ++i) P->is_ground[ground_ids[i]] = 1;
    P->eps2 = eps * eps;
    P->side = eps * (1.0 + 1.0 / 1048576.0);
    return true;
}

template <typename T>
int ext_launch(const T* pts, int64_t n, int dim, const void* labels, int label_bytes, const ExtractParams& P, int32_t cap,
               int32_t* point_cluster, int32_t* cluster_rows, seg3d_instance_cluster* clusters, int32_t* counts, const ExtWs& w,
               hipStream_t st) {
    SEG3D_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), st));
    if (n == 0) return SEG3D_OK;
    const dim3 grid((unsigned)ceil_div64(n, kThreads)), block(kThreads);
    hipLaunchKernelGGL(ext_keys_kernel<T>, grid, block, 0, st, pts, n, dim, labels, label_bytes, P, w.keys[0], w.rows[0],
                       w.keys[2], w.rows[2], w.parent, point_cluster, counts);
    SEG3D_CHECK_LAUNCH();
    rocprim::double_buffer<uint64_t> kb(w.keys[0], w.keys[1]);
    rocprim::double_buffer<uint32_t> vb(w.rows[0], w.rows[1]);
    size_t bytes = w.sort_tmp_bytes;
    SEG3D_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, bytes, kb, vb, (size_t)n, 0u, kCellKeyBits, st));
    const uint64_t* skeys = kb.current();
    const uint32_t* srows = vb.current();
    hipLaunchKernelGGL(ext_core_kernel<T>, grid, block, 0, st, pts, n, dim, P, skeys, srows, w.parent);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(ext_unite_kernel<T>, grid, block, 0, st, pts, n, dim, P, skeys, srows, w.parent);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(ext_label_kernel<T>, grid, block, 0, st, pts, n, dim, P, skeys, srows, w.parent, w.keys[2]);
    SEG3D_CHECK_LAUNCH();
    rocprim::double_buffer<uint64_t> rk(w.keys[2], w.keys[3]);
    rocprim::double_buffer<uint32_t> rv(w.rows[2], w.rows[3]);
    bytes = w.sort_tmp_bytes;
    SEG3D_CHECK_HIP(rocprim::radix_sort_pairs(w.sort_tmp, bytes, rk, rv, (size_t)n, 0u, kRootKeyBits, st));
    const uint64_t* rkeys = rk.current();
    hipLaunchKernelGGL(ext_heads_kernel, grid, block, 0, st, rkeys, n, w.flags, counts);
    SEG3D_CHECK_LAUNCH();
    const int rc = scan_exclusive_u32(w.flags, w.excl, n, reinterpret_cast<uint32_t*>(counts), w.scan_tmp, st);
    if (rc != SEG3D_OK) return rc;
    hipLaunchKernelGGL(ext_emit_kernel, grid, block, 0, st, rkeys, rv.current(), n, w.flags, w.excl, cap, point_cluster,
                       cluster_rows, w.cbegin);
    SEG3D_CHECK_LAUNCH();
    if (cap == 0) return SEG3D_OK;
    hipLaunchKernelGGL(ext_stats_kernel<T>, dim3((unsigned)(cap < kMaxStatBlocks ? cap : kMaxStatBlocks)), block, 0, st, pts, dim,
                       P, rkeys, cluster_rows, w.cbegin, counts, cap, clusters);
    SEG3D_CHECK_LAUNCH();
    const int64_t nb64 = ceil_div64(n, kThreads);
    const int nb = (int)(nb64 > kMaxGroundBlocks ? kMaxGroundBlocks : nb64);
    hipLaunchKernelGGL(ext_ground_kernel<T>, dim3((unsigned)nb, (unsigned)ceil_div64(cap, kChunk)), block, 0, st, pts, n, dim,
                       labels, label_bytes, P, counts, cap, clusters, w.recs);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(ext_fold_kernel<T>, dim3((unsigned)ceil_div64(cap, kThreads)), block, 0, st, pts, dim, counts, cap, nb,
                       w.recs, clusters);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

// ------------------------------------------------------------------------------------------ host twin
int32_t find_host(std::vector<int32_t>& parent, int32_t x) {
    while (parent[x] != x) x = parent[x];
    return x;
}

template <typename T>
void ext_host(const T* pts, int64_t n, int dim, const void* labels, int label_bytes, const ExtractParams& P, int32_t cap,
              int32_t* point_cluster, int32_t* cluster_rows, seg3d_instance_cluster* clusters, int32_t* counts) {
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    std::vector<std::pair<uint64_t, uint32_t>> cells;
    for (int64_t i = 0; i < n; ++i) {
        point_cluster[i] = -1;
        cluster_rows[i] = -1;
        const int64_t l = label_at(labels, label_bytes, i);
        if (l < 0 || l > 255 || P.slot_of[l] == 0xFF) continue;
        cells.emplace_back(make_key(P.slot_of[l], cell_of((double)pts[i * dim], P.side), cell_of((double)pts[i * dim + 1], P.side)),
                           (uint32_t)i);
    }
    const int64_t nt = (int64_t)cells.size();
    counts[3] = (int32_t)nt;
    std::sort(cells.begin(), cells.end());
    std::vector<uint64_t> skeys((size_t)nt + 1);
    std::vector<uint32_t> srows((size_t)nt + 1);
    for (int64_t q = 0; q < nt; ++q) skeys[q] = cells[q].first, srows[q] = cells[q].second;
    std::vector<int32_t> parent((size_t)n + 1, -1);
    for (int64_t q = 0; q < nt; ++q) {
        const int64_t i = srows[q];
        const int need = P.min_points[skeys[q] >> (2 * kCellBits)];
        int cnt = 0;
        for_each_neighbour(skeys.data(), srows.data(), nt, pts, dim, skeys[q], (double)pts[i * dim], (double)pts[i * dim + 1],
                           P.eps2, [&](int32_t) { return ++cnt < need; });
        if (cnt >= need) parent[i] = (int32_t)i;
    }
    std::vector<uint8_t> core((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) core[i] = parent[i] >= 0;
    for (int64_t q = 0; q < nt; ++q) {
        const int32_t i = (int32_t)srows[q];
        if (!core[i]) continue;
        for_each_neighbour(skeys.data(), srows.data(), nt, pts, dim, skeys[q], (double)pts[(int64_t)i * dim],
                           (double)pts[(int64_t)i * dim + 1], P.eps2, [&](int32_t j) {
                               if (j < i && core[j]) {
                                   int32_t a = find_host(parent, i), b = find_host(parent, j);
                                   if (a != b) parent[a > b ? a : b] = a > b ? b : a;
                               }
                               return true;
                           });
    }
    std::vector<std::pair<uint64_t, uint32_t>> rooted;  // ((slot, root), row) of every clustered row
    for (int64_t q = 0; q < nt; ++q) {
        const int32_t i = (int32_t)srows[q];
        int32_t root = kNoRow;
        if (core[i]) {
            root = find_host(parent, i);
        } else {
            for_each_neighbour(skeys.data(), srows.data(), nt, pts, dim, skeys[q], (double)pts[(int64_t)i * dim],
                               (double)pts[(int64_t)i * dim + 1], P.eps2, [&](int32_t j) {
                                   if (core[j]) {
                                       const int32_t r = find_host(parent, j);
                                       root = r < root ? r : root;
                                   }
                                   return true;
                               });
        }
        if (root != kNoRow) rooted.emplace_back(((skeys[q] >> (2 * kCellBits)) << 32) | (uint64_t)(uint32_t)root, (uint32_t)i);
    }
    std::sort(rooted.begin(), rooted.end());
    const int64_t nc = (int64_t)rooted.size();
    counts[2] = (int32_t)nc;
    std::vector<int32_t> ground;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = label_at(labels, label_bytes, i);
        if (l >= 0 && l < 256 && P.is_ground[l]) ground.push_back((int32_t)i);
    }
    int32_t c = -1;
    for (int64_t q = 0; q < nc;) {
        int64_t e = q;
        while (e < nc && rooted[e].first == rooted[q].first) ++e;
        ++c;
        for (int64_t j = q; j < e; ++j) {
            cluster_rows[j] = (int32_t)rooted[j].second;
            point_cluster[rooted[j].second] = c;
        }
        if (c < cap) {
            const int32_t m = (int32_t)(e - q);
            std::vector<double> part(3 * kThreads, 0.0);
            for (int j = 0; j < m; ++j)
                for (int a = 0; a < 3; ++a) part[a * kThreads + j % kThreads] += (double)pts[(int64_t)rooted[q + j].second * dim + a];
            seg3d_instance_cluster o;
            sum3_host(part, o.center);
            for (int a = 0; a < 3; ++a) o.center[a] /= (double)m;
            double r = 0.0;
            for (int j = 0; j < m; ++j) {
                const T* row = pts + (int64_t)rooted[q + j].second * dim;
                const double d = dist3((double)row[0], (double)row[1], (double)row[2], o.center);
                if (d > r) r = d;
            }
            double bd = INFINITY;
            int32_t brow = kNoRow;
            for (const int32_t gi : ground) {
                const T* row = pts + (int64_t)gi * dim;
                const double d = dist3((double)row[0], (double)row[1], (double)row[2], o.center);
                if (closer(d, gi, bd, brow)) bd = d, brow = gi;
            }
            o.label = P.label_of[rooted[q].first >> 32];
            o.begin = (int32_t)q;
            o.rows = m;
            o.radius = r;
            o.kept = (brow != kNoRow && bd < 1.2 * r) ? 1 : 0;
            o.height = o.kept ? o.center[2] - (double)pts[(int64_t)brow * dim + 2] : 0.0;
            counts[1] += o.kept;
            clusters[c] = o;
        }
        q = e;
    }
    counts[0] = c + 1;
}

}  // namespace

extern "C" {

size_t seg3d_instance_extract_workspace_bytes(int64_t n, int32_t cap_clusters) {
    if (n < 0 || n > INT32_MAX - 1 || cap_clusters < 0 || cap_clusters > kMaxCap) return 0;
    ExtWs w;
    size_t bytes = 0;
    if (!ext_carve(nullptr, n, cap_clusters, &w, &bytes)) return 0;
    return bytes + 256;
}

int seg3d_instance_extract(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                           int32_t label_bytes, const uint8_t* target_ids, const int32_t* min_points, int32_t k,
                           const uint8_t* ground_ids, int32_t g, double eps, int32_t cap_clusters, int32_t* point_cluster,
                           int32_t* cluster_rows, seg3d_instance_cluster* clusters, int32_t* counts, void* workspace,
                           size_t workspace_bytes, void* stream) {
    ExtractParams P;
    if (!ext_args_ok(points, n, dim, point_bytes, labels, label_bytes, target_ids, min_points, k, ground_ids, g, eps,
                     cap_clusters, point_cluster, cluster_rows, clusters, counts, &P) ||
        !workspace)
        return SEG3D_EINVAL;
    const size_t need = seg3d_instance_extract_workspace_bytes(n, cap_clusters);
    if (need == 0 || workspace_bytes < need) return SEG3D_EWORKSPACE;
    ExtWs w;
    if (!ext_carve(workspace, n, cap_clusters, &w, nullptr)) return SEG3D_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    if (point_bytes == 4)
        return ext_launch<float>(static_cast<const float*>(points), n, dim, labels, label_bytes, P, cap_clusters, point_cluster,
                                 cluster_rows, clusters, counts, w, st);
    return ext_launch<double>(static_cast<const double*>(points), n, dim, labels, label_bytes, P, cap_clusters, point_cluster,
                              cluster_rows, clusters, counts, w, st);
}

int seg3d_instance_extract_host(const void* points, int64_t n, int32_t dim, int32_t point_bytes, const void* labels,
                                int32_t label_bytes, const uint8_t* target_ids, const int32_t* min_points, int32_t k,
                                const uint8_t* ground_ids, int32_t g, double eps, int32_t cap_clusters,
                                int32_t* point_cluster, int32_t* cluster_rows, seg3d_instance_cluster* clusters,
                                int32_t* counts) {
    ExtractParams P;
    if (!ext_args_ok(points, n, dim, point_bytes, labels, label_bytes, target_ids, min_points, k, ground_ids, g, eps,
                     cap_clusters, point_cluster, cluster_rows, clusters, counts, &P))
        return SEG3D_EINVAL;
    if (point_bytes == 4)
        ext_host<float>(static_cast<const float*>(points), n, dim, labels, label_bytes, P, cap_clusters, point_cluster,
                        cluster_rows, clusters, counts);
    else
        ext_host<double>(static_cast<const double*>(points), n, dim, labels, label_bytes, P, cap_clusters, point_cluster,
                         cluster_rows, clusters, counts);
    return SEG3D_OK;
}

}  // extern "C"
