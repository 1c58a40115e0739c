// Training augmentation on the device: PolarMix, the global transforms, PointShuffle / PointSample.
// Reference: seg3d/datasets/transforms/polarmix.py:4-111 (swap, rotate_copy, PolarMix.__call__),
// transforms.py:79-258 (RandomGlobalRotation / Scaling / Translation, RandomFlip, PointShuffle, PointSample),
// transform_utils.py:11-138, composed at seg3d/datasets/waymo_dataset.py:44-50 and called at :262-263, :307-323.
//
// MI355X design: every stage of that pipeline either selects / reorders rows or applies one affine map per row, so the
// reference's ~ten host copies of the [N, D] frame become (1) a chain of small int32 kernels that composes a source
// map (flags -> scan -> emit; sorts of hashed keys for the device-side shuffle / sample) and (2) ONE gather-and-
// transform kernel that reads every source row once and writes every final row once; labels and image features go
// through the same map.  Nothing here allocates or synchronises; no float atomics, so every output is reproducible.
// Each device entry has a host twin below it: plain C++ that makes no HIP call and shares the per-row recipes.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"

// the per-row recipe is a fixed sequence of IEEE products and sums (numpy / torch round each of them); a fused
// multiply-add would change the last bit against the host twin and the reference
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxDim = 16;

// ------------------------------------------------------------------------------------------ shared recipes
// polarmix.py:7-12: yaw = -arctan2(y, x), strictly inside (alpha, beta); evaluated in double
__host__ __device__ __forceinline__ bool in_sector(double x, double y, double alpha, double beta) {
    const double yaw = -atan2(y, x);
    return yaw > alpha && yaw < beta;
}

// One output row's x, y, z from its source row.  op > 0: polarmix.py:48-53 (np.dot with the float64 matrix
// [[c, s, 0], [-s, c, 0], [0, 0, 1]], in double), then the `.float()` of transform_utils.py:7; then in float32
// transform_utils.py:11-32 (points @ R), transforms.py:87 (xyz *= float32 scale), transform_utils.py:68-94 (the float64
// offset added in double and rounded once), :35-58 (flip_x negates y, then flip_y negates x).
template <typename T>
__host__ __device__ __forceinline__ void aug_point(const seg3d_aug_params& p, int op, T xi, T yi, T zi, float* o) {
    float x, y, z = (float)zi;
    if (op > 0) {
        const double c = p.paste_cos[op - 1], s = p.paste_sin[op - 1];
        const double xd = (double)xi, yd = (double)yi;
        x = (float)(xd * c + yd * (-s));
        y = (float)(xd * s + yd * c);
    } else {
        x = (float)xi;
        y = (float)yi;
    }
    if (p.global_on) {
        const float xr = x * p.rot_cos + y * (-p.rot_sin);
        const float yr = x * p.rot_sin + y * p.rot_cos;
        x = xr * p.scale;
        y = yr * p.scale;
        z = z * p.scale;
        x = (float)((double)x + p.offset[0]);
        y = (float)((double)y + p.offset[1]);
        z = (float)((double)z + p.offset[2]);
        if (p.flip_x) y = -y;
        if (p.flip_y) x = -x;
    }
    o[0] = x;
    o[1] = y;
    o[2] = z;
}

// transform_utils.py:122-124: np.linalg.norm of the float32 x, y (two rounded products, a rounded sum, IEEE sqrt)
__host__ __device__ __forceinline__ bool is_far(float x, float y, float range) {
    const float d = sqrtf(x * x + y * y);
    return d >= range;
}

// row s of the concatenation [frame1; frame2], or NULL when s is not a row of it
template <typename T>
__host__ __device__ __forceinline__ const T* cat_row(const T* f1, int64_t n1, const T* f2, int64_t n2, int64_t s,
                                                     int dim) {
    if (s < 0 || s >= n1 + n2) return nullptr;
    return s < n1 ? f1 + s * dim : f2 + (s - n1) * dim;
}

// counter-based hash of (seed, stream, row): the splitmix64 finaliser over a mixed counter
__host__ __device__ __forceinline__ uint64_t aug_hash(uint64_t seed, uint32_t stream, uint32_t row) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (((uint64_t)stream << 32 | row) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// selection key: far rows (bit 63 clear) sort in front of near rows, a 31-bit hash orders each set, the row makes it unique
__host__ __device__ __forceinline__ uint64_t select_key(uint64_t seed, uint32_t row, bool far) {
    return ((uint64_t)(far ? 0 : 1) << 63) | ((aug_hash(seed, 1u, row) >> 33) << 32) | row;
}

// order key of a kept row: a fresh 32-bit hash, the row makes it unique
__host__ __device__ __forceinline__ uint64_t order_key(uint64_t seed, uint32_t row) {
    return ((aug_hash(seed, 2u, row) >> 32) << 32) | row;
}

struct ClassSlots {
    uint8_t slot[256];  // position of a label in instance_classes, 255 = not an instance class
};

__host__ __device__ __forceinline__ int label_slot(const ClassSlots& cs, const void* labels, int label_bytes, int64_t j) {
    if (label_bytes == 1) return cs.slot[static_cast<const uint8_t*>(labels)[j]];
    const int64_t l = static_cast<const int64_t*>(labels)[j];
    return (l >= 0 && l < 256) ? cs.slot[l] : 255;
}

bool make_slots(const uint8_t* classes, int32_t n_classes, ClassSlots* cs) {
    if (n_classes < 0 || n_classes > 255 || (n_classes > 0 && !classes)) return false;
    memset(cs->slot, 255, sizeof(cs->slot));
    for (int k = 0; k < n_classes; ++k) {
        if (cs->slot[classes[k]] != 255) return false;  // a class listed twice
        cs->slot[classes[k]] = (uint8_t)k;
    }
    return true;
}

bool params_ok(const seg3d_aug_params* p) {
    if (!p || p->n_paste < 0 || p->n_paste > SEG3D_AUG_MAX_PASTE) return false;
    return (p->flip_x == 0 || p->flip_x == 1) && (p->flip_y == 0 || p->flip_y == 1) &&
           (p->global_on == 0 || p->global_on == 1) && (p->batch_col == 0 || p->batch_col == 1);
}

// ------------------------------------------------------------------------------------------ (1) PolarMix map
template <typename T>
__global__ __launch_bounds__(kThreads) void pm_flags_kernel(const T* __restrict__ p1, int64_t n1, const T* __restrict__ p2,
                                                            int64_t n2, int dim, int swap, double alpha, double beta,
                                                            uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n1 + n2) return;
    const T* row = i < n1 ? p1 + i * dim : p2 + (i - n1) * dim;
    const bool in = swap && in_sector((double)row[0], (double)row[1], alpha, beta);
    flag[i] = (i < n1 ? !in : in) ? 1u : 0u;  // frame 1 keeps what lies outside, frame 2 gives what lies inside
}

__global__ __launch_bounds__(kThreads) void pm_emit_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                           int64_t n, int64_t cap, int32_t* __restrict__ src,
                                                           uint8_t* __restrict__ op) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t o = pos[i];
    if (o >= cap) return;
    src[o] = (int32_t)i;
    op[o] = 0;
}

// per-block histogram of the instance-class slots of frame 2, laid out class-major: hist[slot * nb + block]
__global__ __launch_bounds__(kThreads) void pm_inst_hist_kernel(const void* __restrict__ labels, int label_bytes, int64_t n2,
                                                                ClassSlots cs, int n_classes, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < n2) {
        const int s = label_slot(cs, labels, label_bytes, j);
        if (s < n_classes) atomicAdd(&lh[s], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < n_classes) hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = lh[threadIdx.x];
}

// stable rank inside the block + scanned histogram = the row's place in the class-major instance block
// (polarmix.py:31-41); the block is written 1 + R times: unrotated, then once per paste angle (:44-58)
__global__ __launch_bounds__(kThreads) void pm_inst_emit_kernel(const void* __restrict__ labels, int label_bytes, int64_t n1,
                                                                int64_t n2, ClassSlots cs, int n_classes, int n_paste,
                                                                const uint32_t* __restrict__ hoffs,
                                                                const uint32_t* __restrict__ totals, int64_t cap,
                                                                int32_t* __restrict__ src, uint8_t* __restrict__ op) {
    __shared__ uint8_t ls[kThreads];
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int s = j < n2 ? label_slot(cs, labels, label_bytes, j) : 255;
    ls[threadIdx.x] = (uint8_t)s;
    __syncthreads();
    if (s >= n_classes) return;
    uint32_t r = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) r += ls[t] == (uint8_t)s ? 1u : 0u;
    const int64_t base = totals[0], n_inst = totals[1];
    const int64_t k = (int64_t)hoffs[(int64_t)s * gridDim.x + blockIdx.x] + r;
    for (int a = 0; a <= n_paste; ++a) {
        const int64_t o = base + (int64_t)a * n_inst + k;
        if (o >= cap) return;
        src[o] = (int32_t)(n1 + j);
        op[o] = (uint8_t)a;
    }
}

__global__ void pm_counts_kernel(const uint32_t* __restrict__ totals, int n_paste, int32_t* __restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = (int32_t)(totals[0] + (uint32_t)(1 + n_paste) * totals[1]);
        counts[1] = (int32_t)totals[0];
        counts[2] = (int32_t)totals[1];
        counts[3] = 0;
    }
}

struct PmWs {
    uint32_t *flag, *pos, *tmp, *totals, *hist, *hoffs, *htmp;
};

int64_t pm_blocks(int64_t n2) { return ceil_div64(n2 > 0 ? n2 : 1, kThreads); }

PmWs pm_carve(void* ws, int64_t n1, int64_t n2, size_t* bytes) {
    WsCarver c(ws);
    PmWs w;
    const size_t n = (size_t)(n1 + n2), nh = (size_t)pm_blocks(n2) * 255;
    w.flag = c.take<uint32_t>(n + 1);
    w.pos = c.take<uint32_t>(n + 1);
    w.tmp = c.take<uint32_t>(scan_tmp_count((int64_t)n));
    w.totals = c.take<uint32_t>(4);
    w.hist = c.take<uint32_t>(nh);
    w.hoffs = c.take<uint32_t>(nh);
    w.htmp = c.take<uint32_t>(scan_tmp_count((int64_t)nh));
    if (bytes) *bytes = c.off;
    return w;
}

bool pm_args_ok(const void* p1, int64_t n1, const void* p2, int64_t n2, int32_t dim, int32_t point_bytes,
                const void* labels2, int32_t label_bytes, int32_t swap, int32_t n_paste, int64_t cap, const void* src,
                const void* op, const void* counts) {
    if (n1 < 0 || n2 < 0 || dim < 3 || dim > kMaxDim || (point_bytes != 4 && point_bytes != 8)) return false;
    if (label_bytes != 1 && label_bytes != 8) return false;
    if ((swap != 0 && swap != 1) || n_paste < 0 || n_paste > SEG3D_AUG_MAX_PASTE || !counts) return false;
    if (n1 > INT32_MAX / 4 || n2 > INT32_MAX / 16) return false;  // n1 + n2 * (2 + R) rows indexed in int32
    if (cap < n1 + n2 * (2 + (int64_t)n_paste)) return false;
    if ((n1 > 0 && !p1) || (n2 > 0 && (!p2 || !labels2))) return false;
    if (cap > 0 && (!src || !op)) return false;
    return true;
}

template <typename T>
int pm_launch(const T* p1, int64_t n1, const T* p2, int64_t n2, int dim, const void* labels2, int label_bytes, int swap,
              double alpha, double beta, const ClassSlots& cs, int n_classes, int n_paste, int64_t cap, int32_t* src,
              uint8_t* op, int32_t* counts, void* workspace, hipStream_t st) {
    PmWs w = pm_carve(workspace, n1, n2, nullptr);
    const int64_t n = n1 + n2, nb2 = pm_blocks(n2), nh = nb2 * n_classes;
    if (n > 0) {
        const unsigned nb = (unsigned)ceil_div64(n, kThreads);
        hipLaunchKernelGGL(pm_flags_kernel<T>, dim3(nb), dim3(kThreads), 0, st, p1, n1, p2, n2, dim, swap, alpha, beta,
                           w.flag);
        SEG3D_CHECK_LAUNCH();
    }
    int rc = scan_exclusive_u32(w.flag, w.pos, n, w.totals, w.tmp, st);
    if (rc != SEG3D_OK) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(pm_emit_kernel, dim3((unsigned)ceil_div64(n, kThreads)), dim3(kThreads), 0, st, w.flag, w.pos, n,
                           cap, src, op);
        SEG3D_CHECK_LAUNCH();
    }
    if (n2 > 0 && n_classes > 0) {
        hipLaunchKernelGGL(pm_inst_hist_kernel, dim3((unsigned)nb2), dim3(kThreads), 0, st, labels2, label_bytes, n2, cs,
                           n_classes, w.hist);
        SEG3D_CHECK_LAUNCH();
    }
    rc = scan_exclusive_u32(w.hist, w.hoffs, (n2 > 0 ? nh : 0), w.totals + 1, w.htmp, st);
    if (rc != SEG3D_OK) return rc;
    if (n2 > 0 && n_classes > 0) {
        hipLaunchKernelGGL(pm_inst_emit_kernel, dim3((unsigned)nb2), dim3(kThreads), 0, st, labels2, label_bytes, n1, n2,
                           cs, n_classes, n_paste, w.hoffs, w.totals, cap, src, op);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pm_counts_kernel, dim3(1), dim3(64), 0, st, w.totals, n_paste, counts);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

template <typename T>
void pm_host(const T* p1, int64_t n1, const T* p2, int64_t n2, int dim, const void* labels2, int label_bytes, int swap,
             double alpha, double beta, const ClassSlots& cs, int n_classes, int n_paste, int32_t* src, uint8_t* op,
             int32_t* counts) {
    int64_t o = 0;
    for (int64_t i = 0; i < n1; ++i)
        if (!(swap && in_sector((double)p1[i * dim], (double)p1[i * dim + 1], alpha, beta))) {
            src[o] = (int32_t)i;
            op[o++] = 0;
        }
    for (int64_t j = 0; j < n2; ++j)
        if (swap && in_sector((double)p2[j * dim], (double)p2[j * dim + 1], alpha, beta)) {
            src[o] = (int32_t)(n1 + j);
            op[o++] = 0;
        }
    const int64_t base = o;
    for (int k = 0; k < n_classes; ++k)
        for (int64_t j = 0; j < n2; ++j)
            if (label_slot(cs, labels2, label_bytes, j) == k) {
                src[o] = (int32_t)(n1 + j);
                op[o++] = 0;
            }
    const int64_t n_inst = o - base;
    for (int a = 1; a <= n_paste; ++a)
        for (int64_t k = 0; k < n_inst; ++k) {
            src[o] = src[base + k];
            op[o++] = (uint8_t)a;
        }
    counts[0] = (int32_t)o;
    counts[1] = (int32_t)base;
    counts[2] = (int32_t)n_inst;
    counts[3] = 0;
}

// ------------------------------------------------------------------------------------------ (2a) far / near lists
// far flag of row i of the transformed, shuffled frame: source row src[idx[i]] (idx NULL: src[i]; src NULL: row itself)
template <typename T>
__host__ __device__ __forceinline__ bool far_of_row(const T* f1, int64_t n1, const T* f2, int64_t n2, int dim,
                                                    const int32_t* src, const uint8_t* op, int64_t n_map,
                                                    const int32_t* idx, int64_t i, const seg3d_aug_params& p, float range) {
    int64_t m = idx ? idx[i] : i;
    if (m < 0 || m >= n_map) return false;
    const int64_t s = src ? src[m] : m;
    int k = op ? op[m] : 0;
    if (k > p.n_paste) k = 0;
    const T* row = cat_row(f1, n1, f2, n2, s, dim);
    if (!row) return false;
    float o[3];
    aug_point<T>(p, k, row[0], row[1], row[2], o);
    return is_far(o[0], o[1], range);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void far_flags_kernel(const T* __restrict__ f1, int64_t n1, const T* __restrict__ f2,
                                                             int64_t n2, int dim, const int32_t* __restrict__ src,
                                                             const uint8_t* __restrict__ op, int64_t n_map,
                                                             const int32_t* __restrict__ idx, int64_t n, seg3d_aug_params p,
                                                             float range, uint32_t* __restrict__ flag,
                                                             uint8_t* __restrict__ flag8) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const bool far = far_of_row<T>(f1, n1, f2, n2, dim, src, op, n_map, idx, i, p, range);
    if (flag) flag[i] = far ? 1u : 0u;
    if (flag8) flag8[i] = far ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void far_emit_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ total, int64_t n,
                                                            int32_t* __restrict__ far, int32_t* __restrict__ near,
                                                            int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) {
        counts[0] = (int32_t)*total;
        counts[1] = (int32_t)(n - (int64_t)*total);
    }
    if (i >= n) return;
    if (flag[i])
        far[pos[i]] = (int32_t)i;
    else
        near[i - pos[i]] = (int32_t)i;
}

struct FarWs {
    uint32_t *flag, *pos, *tmp, *total;
};

FarWs far_carve(void* ws, int64_t n, size_t* bytes) {
    WsCarver c(ws);
    FarWs w;
    w.flag = c.take<uint32_t>((size_t)n + 1);
    w.pos = c.take<uint32_t>((size_t)n + 1);
    w.tmp = c.take<uint32_t>(scan_tmp_count(n));
    w.total = c.take<uint32_t>(4);
    if (bytes) *bytes = c.off;
    return w;
}

bool far_args_ok(const void* f1, int64_t n1, const void* f2, int64_t n2, int32_t dim, int32_t point_bytes, int64_t n_map,
                 int64_t n, const seg3d_aug_params* p) {
    if (n1 < 0 || n2 < 0 || n_map < 0 || n < 0 || dim < 3 || dim > kMaxDim || (point_bytes != 4 && point_bytes != 8))
        return false;
    if (n1 + n2 > INT32_MAX || n_map > INT32_MAX || n > INT32_MAX || !params_ok(p)) return false;
    if ((n1 > 0 && !f1) || (n2 > 0 && !f2)) return false;
    return true;
}

template <typename T>
int far_launch(const T* f1, int64_t n1, const T* f2, int64_t n2, int dim, const int32_t* src, const uint8_t* op,
               int64_t n_map, const int32_t* idx, int64_t n, const seg3d_aug_params& p, float range, uint8_t* far_flag,
               int32_t* far, int32_t* near, int32_t* counts, void* workspace, hipStream_t st) {
    FarWs w = far_carve(workspace, n, nullptr);
    const bool lists = far != nullptr;
    const unsigned nb = (unsigned)ceil_div64(n > 0 ? n : 1, kThreads);
    if (n > 0) {
        hipLaunchKernelGGL(far_flags_kernel<T>, dim3(nb), dim3(kThreads), 0, st, f1, n1, f2, n2, dim, src, op, n_map, idx,
                           n, p, range, lists ? w.flag : nullptr, far_flag);
        SEG3D_CHECK_LAUNCH();
    }
    if (!lists) return SEG3D_OK;
    const int rc = scan_exclusive_u32(w.flag, w.pos, n, w.total, w.tmp, st);
    if (rc != SEG3D_OK) return rc;
    hipLaunchKernelGGL(far_emit_kernel, dim3(nb), dim3(kThreads), 0, st, w.flag, w.pos, w.total, n, far, near, counts);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

template <typename T>
void far_host(const T* f1, int64_t n1, const T* f2, int64_t n2, int dim, const int32_t* src, const uint8_t* op,
              int64_t n_map, const int32_t* idx, int64_t n, const seg3d_aug_params& p, float range, uint8_t* far_flag,
              int32_t* far, int32_t* near, int32_t* counts) {
    int64_t nf = 0, nn = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool f = far_of_row<T>(f1, n1, f2, n2, dim, src, op, n_map, idx, i, p, range);
        if (far_flag) far_flag[i] = f ? 1 : 0;
        if (far) {
            if (f)
                far[nf++] = (int32_t)i;
            else
                near[nn++] = (int32_t)i;
        }
    }
    if (far) {
        counts[0] = (int32_t)nf;
        counts[1] = (int32_t)nn;
    }
}

// ------------------------------------------------------------------------------------------ (2b) device-side sample
__global__ __launch_bounds__(kThreads) void select_keys_kernel(const uint8_t* __restrict__ far_flag, int64_t n, uint64_t seed,
                                                               unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) keys[i] = select_key(seed, (uint32_t)i, far_flag ? far_flag[i] != 0 : false);
}

__global__ __launch_bounds__(kThreads) void order_keys_kernel(const unsigned long long* __restrict__ sorted, int64_t m,
                                                              uint64_t seed, unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < m) keys[i] = order_key(seed, (uint32_t)(sorted[i] & 0xFFFFFFFFull));
}

__global__ __launch_bounds__(kThreads) void key_rows_kernel(const unsigned long long* __restrict__ sorted, int64_t m,
                                                            int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < m) out[i] = (int32_t)(sorted[i] & 0xFFFFFFFFull);
}

bool sort_tmp_bytes(int64_t n, size_t* bytes) {
    *bytes = 0;
    if (n == 0) return true;
    unsigned long long* none = nullptr;
    return rocprim::radix_sort_keys(nullptr, *bytes, none, none, (size_t)n, 0u, 64u) == hipSuccess;
}

struct SampleWs {
    unsigned long long *k0, *k1;
    void* tmp;
    size_t tmp_bytes;
};

bool sample_carve(void* ws, int64_t n, SampleWs* w, size_t* bytes) {
    if (!sort_tmp_bytes(n, &w->tmp_bytes)) return false;
    WsCarver c(ws);
    w->k0 = c.take<unsigned long long>((size_t)n + 1);
    w->k1 = c.take<unsigned long long>((size_t)n + 1);
    w->tmp = c.take<char>(w->tmp_bytes + 1);
    if (bytes) *bytes = c.off;
    return true;
}

// ------------------------------------------------------------------------------------------ (2c) multi-sweep map
__global__ __launch_bounds__(kThreads) void cur_scatter_kernel(const int32_t* __restrict__ cur, int64_t nc, int64_t n_points,
                                                               int32_t* __restrict__ inv) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nc) return;
    const int32_t p = cur[i];
    if (p >= 0 && p < n_points) atomicMax(&inv[p], (int32_t)i);  // a point listed twice: the later slot, as the dict keeps
}

__global__ __launch_bounds__(kThreads) void cur_flags_kernel(const int32_t* __restrict__ src, int64_t m, int64_t n_points,
                                                             const int32_t* __restrict__ inv, uint32_t* __restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= m) return;
    const int32_t s = src[k];
    flag[k] = (s >= 0 && s < n_points && inv[s] >= 0) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void cur_emit_kernel(const int32_t* __restrict__ src, int64_t m,
                                                            const int32_t* __restrict__ inv, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                            int32_t* __restrict__ cur_pos, int32_t* __restrict__ cur_gather,
                                                            int32_t* __restrict__ count) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k == 0) count[0] = (int32_t)*total;
    if (k >= m || !flag[k]) return;
    cur_pos[pos[k]] = (int32_t)k;
    cur_gather[pos[k]] = inv[src[k]];
}

struct CurWs {
    int32_t* inv;
    uint32_t *flag, *pos, *tmp, *total;
};

CurWs cur_carve(void* ws, int64_t m, int64_t n_points, size_t* bytes) {
    WsCarver c(ws);
    CurWs w;
    w.inv = c.take<int32_t>((size_t)n_points + 1);
    w.flag = c.take<uint32_t>((size_t)m + 1);
    w.pos = c.take<uint32_t>((size_t)m + 1);
    w.tmp = c.take<uint32_t>(scan_tmp_count(m));
    w.total = c.take<uint32_t>(4);
    if (bytes) *bytes = c.off;
    return w;
}

// ------------------------------------------------------------------------------------------ (3) apply
template <int D, typename T>
__device__ __forceinline__ void load_row(const T* __restrict__ row, bool aligned16, T* in) {
    constexpr int kRowBytes = D * (int)sizeof(T);
    if constexpr (kRowBytes % 16 == 0) {
        if (aligned16) {  // every row of a 16-B aligned frame starts on a 16-B boundary
            constexpr int kPer = 16 / (int)sizeof(T);
            using V = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
            const V* r = reinterpret_cast<const V*>(row);
#pragma unroll
            for (int q = 0; q < kRowBytes / 16; ++q) {
                const V v = r[q];
                const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
                for (int c = 0; c < kPer; ++c) in[q * kPer + c] = e[c];
            }
            return;
        }
    } else if constexpr (kRowBytes % 8 == 0 && sizeof(T) == 4) {
        if (aligned16) {
            const float2* r = reinterpret_cast<const float2*>(row);
#pragma unroll
            for (int q = 0; q < D / 2; ++q) {
                const float2 v = r[q];
                in[2 * q] = v.x;
                in[2 * q + 1] = v.y;
            }
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < D; ++c) in[c] = row[c];
}

// one thread = four consecutive output rows: their 4 * W floats start on a 16-B boundary for every W, so the stores are
// W float4 when `out` is 16-B aligned; each source row is read once, with the widest load its alignment allows
template <int D, typename T, int BC>
__global__ __launch_bounds__(kThreads) void aug_apply_kernel(const T* __restrict__ f1, int64_t n1, const T* __restrict__ f2,
                                                             int64_t n2, const int32_t* __restrict__ src,
                                                             const uint8_t* __restrict__ op, int64_t n_out,
                                                             seg3d_aug_params p, int in_al, int out_al,
                                                             float* __restrict__ out) {
    constexpr int W = D + BC;
    const int64_t g0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (g0 >= n_out) return;
    float o[4 * W];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t g = g0 + r;
        T in[D];
#pragma unroll
        for (int c = 0; c < D; ++c) in[c] = (T)0;
        int k = 0;
        if (g < n_out) {
            const int64_t s = src ? (int64_t)src[g] : g;
            k = op ? (int)op[g] : 0;
            if (k > p.n_paste) k = 0;
            const T* row = cat_row(f1, n1, f2, n2, s, D);
            if (row) load_row<D, T>(row, in_al != 0, in);  // a row outside both frames reads as zeros
        }
        if (BC) o[r * W] = p.batch_id;
        aug_point<T>(p, k, in[0], in[1], in[2], &o[r * W + BC]);
#pragma unroll
        for (int c = 3; c < D; ++c) o[r * W + BC + c] = (float)in[c];
    }
    if (out_al && g0 + 4 <= n_out) {
        float4* o4 = reinterpret_cast<float4*>(out + g0 * W);
#pragma unroll
        for (int q = 0; q < W; ++q) o4[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    } else {
        for (int r = 0; r < 4; ++r) {
            if (g0 + r >= n_out) break;
#pragma unroll
            for (int c = 0; c < W; ++c) out[(g0 + r) * W + c] = o[r * W + c];
        }
    }
}

bool apply_args_ok(const void* f1, int64_t n1, const void* f2, int64_t n2, int32_t dim, const int32_t* src, int64_t n_out,
                   const seg3d_aug_params* p, const float* out) {
    if (n1 < 0 || n2 < 0 || n_out < 0 || dim < 3 || dim > kMaxDim || !params_ok(p)) return false;
    if (n1 + n2 > INT32_MAX || n_out > INT32_MAX) return false;
    if ((n1 > 0 && !f1) || (n2 > 0 && !f2) || (n_out > 0 && !out)) return false;
    if (!src && n_out > n1 + n2) return false;
    return true;
}

template <int D, typename T>
void launch_apply(const T* f1, int64_t n1, const T* f2, int64_t n2, const int32_t* src, const uint8_t* op, int64_t n_out,
                  const seg3d_aug_params& p, float* out, hipStream_t st) {
    const int in_al = ((reinterpret_cast<uintptr_t>(f1) | reinterpret_cast<uintptr_t>(f2)) & 15) == 0;
    const int out_al = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const unsigned nb = (unsigned)ceil_div64(ceil_div64(n_out, 4), kThreads);
    if (p.batch_col)
        hipLaunchKernelGGL((aug_apply_kernel<D, T, 1>), dim3(nb), dim3(kThreads), 0, st, f1, n1, f2, n2, src, op, n_out, p,
                           in_al, out_al, out);
    else
        hipLaunchKernelGGL((aug_apply_kernel<D, T, 0>), dim3(nb), dim3(kThreads), 0, st, f1, n1, f2, n2, src, op, n_out, p,
                           in_al, out_al, out);
}

template <typename T>
int apply_device(const T* f1, int64_t n1, const T* f2, int64_t n2, int32_t dim, const int32_t* src, const uint8_t* op,
                 int64_t n_out, const seg3d_aug_params* params, float* out, void* stream) {
    if (!apply_args_ok(f1, n1, f2, n2, dim, src, n_out, params, out)) return SEG3D_EINVAL;
    if (n_out == 0) return SEG3D_OK;
    const seg3d_aug_params p = *params;  // by value into the kernel arguments: no copy to the device
    hipStream_t st = as_stream(stream);
    switch (dim) {
#define SEG3D_APPLY_CASE(d) \
    case d: launch_apply<d, T>(f1, n1, f2, n2, src, op, n_out, p, out, st); break;
        SEG3D_APPLY_CASE(3) SEG3D_APPLY_CASE(4) SEG3D_APPLY_CASE(5) SEG3D_APPLY_CASE(6) SEG3D_APPLY_CASE(7)
        SEG3D_APPLY_CASE(8) SEG3D_APPLY_CASE(9) SEG3D_APPLY_CASE(10) SEG3D_APPLY_CASE(11) SEG3D_APPLY_CASE(12)
        SEG3D_APPLY_CASE(13) SEG3D_APPLY_CASE(14) SEG3D_APPLY_CASE(15) SEG3D_APPLY_CASE(16)
#undef SEG3D_APPLY_CASE
        default: return SEG3D_EINVAL;
    }
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

template <typename T>
int apply_host(const T* f1, int64_t n1, const T* f2, int64_t n2, int32_t dim, const int32_t* src, const uint8_t* op,
               int64_t n_out, const seg3d_aug_params* params, float* out) {
    if (!apply_args_ok(f1, n1, f2, n2, dim, src, n_out, params, out)) return SEG3D_EINVAL;
    const seg3d_aug_params& p = *params;
    const int bc = p.batch_col, w = dim + bc;
    for (int64_t g = 0; g < n_out; ++g) {
        const int64_t s = src ? (int64_t)src[g] : g;
        int k = op ? (int)op[g] : 0;
        if (k > p.n_paste) k = 0;
        T in[kMaxDim];
        const T* row = cat_row(f1, n1, f2, n2, s, dim);
        for (int c = 0; c < dim; ++c) in[c] = row ? row[c] : (T)0;
        float* o = out + g * w;
        if (bc) o[0] = p.batch_id;
        aug_point<T>(p, k, in[0], in[1], in[2], o + bc);
        for (int c = 3; c < dim; ++c) o[bc + c] = (float)in[c];
    }
    return SEG3D_OK;
}

// ------------------------------------------------------------------------------------------ (4) label / feature gather
template <typename U>
__global__ __launch_bounds__(kThreads) void aug_gather_kernel(const U* __restrict__ a, int64_t na, const U* __restrict__ b,
                                                              int64_t nb, int units, const int32_t* __restrict__ idx,
                                                              int64_t total, U* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t g = e / units;
    const int u = (int)(e - g * units);
    const int64_t s = idx[g];
    U v;
    memset(&v, 0, sizeof(U));
    if (s >= 0 && s < na)
        v = a[s * units + u];
    else if (s >= na && s < na + nb)
        v = b[(s - na) * units + u];
    out[e] = v;
}

bool gather_args_ok(const void* a, int64_t na, const void* b, int64_t nb, int64_t row_bytes, const int32_t* idx, int64_t m,
                    const void* out) {
    if (na < 0 || nb < 0 || m < 0 || row_bytes < 1 || row_bytes > 4096) return false;
    if (na + nb > INT32_MAX || m > INT32_MAX) return false;
    if ((na > 0 && !a) || (nb > 0 && !b) || (m > 0 && (!idx || !out))) return false;
    return true;
}

template <typename U>
void launch_gather(const void* a, int64_t na, const void* b, int64_t nb, int64_t row_bytes, const int32_t* idx, int64_t m,
                   void* out, hipStream_t st) {
    const int units = (int)(row_bytes / (int64_t)sizeof(U));
    const int64_t total = m * units;
    hipLaunchKernelGGL(aug_gather_kernel<U>, dim3((unsigned)ceil_div64(total, kThreads)), dim3(kThreads), 0, st,
                       static_cast<const U*>(a), na, static_cast<const U*>(b), nb, units, idx, total,
                       static_cast<U*>(out));
}

}  // namespace

extern "C" {

size_t seg3d_aug_polarmix_workspace_bytes(int64_t n1, int64_t n2) {
    size_t bytes = 0;
    pm_carve(nullptr, n1 > 0 ? n1 : 0, n2 > 0 ? n2 : 0, &bytes);
    return bytes;
}

int seg3d_aug_polarmix_map(const void* points1, int64_t n1, const void* points2, int64_t n2, int32_t dim,
                           int32_t point_bytes, const void* labels2, int32_t label_bytes, int32_t swap, double alpha,
                           double beta, const uint8_t* instance_classes, int32_t n_classes, int32_t n_paste, int64_t cap,
                           int32_t* src, uint8_t* op, int32_t* counts, void* workspace, size_t workspace_bytes,
                           void* stream) {
    ClassSlots cs;
    if (!pm_args_ok(points1, n1, points2, n2, dim, point_bytes, labels2, label_bytes, swap, n_paste, cap, src, op, counts) ||
        !make_slots(instance_classes, n_classes, &cs) || !workspace)
        return SEG3D_EINVAL;
    if (workspace_bytes < seg3d_aug_polarmix_workspace_bytes(n1, n2)) return SEG3D_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    if (point_bytes == 4)
        return pm_launch<float>(static_cast<const float*>(points1), n1, static_cast<const float*>(points2), n2, dim, labels2,
                                label_bytes, swap, alpha, beta, cs, n_classes, n_paste, cap, src, op, counts, workspace, st);
    return pm_launch<double>(static_cast<const double*>(points1), n1, static_cast<const double*>(points2), n2, dim, labels2,
                             label_bytes, swap, alpha, beta, cs, n_classes, n_paste, cap, src, op, counts, workspace, st);
}

int seg3d_aug_polarmix_map_host(const void* points1, int64_t n1, const void* points2, int64_t n2, int32_t dim,
                                int32_t point_bytes, const void* labels2, int32_t label_bytes, int32_t swap, double alpha,
                                double beta, const uint8_t* instance_classes, int32_t n_classes, int32_t n_paste,
                                int64_t cap, int32_t* src, uint8_t* op, int32_t* counts) {
    ClassSlots cs;
    if (!pm_args_ok(points1, n1, points2, n2, dim, point_bytes, labels2, label_bytes, swap, n_paste, cap, src, op, counts) ||
        !make_slots(instance_classes, n_classes, &cs))
        return SEG3D_EINVAL;
    if (point_bytes == 4)
        pm_host<float>(static_cast<const float*>(points1), n1, static_cast<const float*>(points2), n2, dim, labels2,
                       label_bytes, swap, alpha, beta, cs, n_classes, n_paste, src, op, counts);
    else
        pm_host<double>(static_cast<const double*>(points1), n1, static_cast<const double*>(points2), n2, dim, labels2,
                        label_bytes, swap, alpha, beta, cs, n_classes, n_paste, src, op, counts);
    return SEG3D_OK;
}

size_t seg3d_aug_far_near_workspace_bytes(int64_t n) {
    size_t bytes = 0;
    far_carve(nullptr, n > 0 ? n : 0, &bytes);
    return bytes;
}

int seg3d_aug_far_near(const void* frame1, int64_t n1, const void* frame2, int64_t n2, int32_t dim, int32_t point_bytes,
                       const int32_t* src, const uint8_t* op, int64_t n_map, const int32_t* idx, int64_t n,
                       const seg3d_aug_params* params, float sample_range, uint8_t* far_flag, int32_t* far_idx,
                       int32_t* near_idx, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!far_args_ok(frame1, n1, frame2, n2, dim, point_bytes, n_map, n, params)) return SEG3D_EINVAL;
    if ((far_idx != nullptr) != (near_idx != nullptr) || (far_idx && !counts) || (!far_idx && !far_flag)) return SEG3D_EINVAL;
    if (!src && n_map > n1 + n2) return SEG3D_EINVAL;
    if (far_idx && !workspace) return SEG3D_EINVAL;
    if (far_idx && workspace_bytes < seg3d_aug_far_near_workspace_bytes(n)) return SEG3D_EWORKSPACE;
    const seg3d_aug_params p = *params;
    hipStream_t st = as_stream(stream);
    if (point_bytes == 4)
        return far_launch<float>(static_cast<const float*>(frame1), n1, static_cast<const float*>(frame2), n2, dim, src, op,
                                 n_map, idx, n, p, sample_range, far_flag, far_idx, near_idx, counts, workspace, st);
    return far_launch<double>(static_cast<const double*>(frame1), n1, static_cast<const double*>(frame2), n2, dim, src, op,
                              n_map, idx, n, p, sample_range, far_flag, far_idx, near_idx, counts, workspace, st);
}

int seg3d_aug_far_near_host(const void* frame1, int64_t n1, const void* frame2, int64_t n2, int32_t dim, int32_t point_bytes,
                            const int32_t* src, const uint8_t* op, int64_t n_map, const int32_t* idx, int64_t n,
                            const seg3d_aug_params* params, float sample_range, uint8_t* far_flag, int32_t* far_idx,
                            int32_t* near_idx, int32_t* counts) {
    if (!far_args_ok(frame1, n1, frame2, n2, dim, point_bytes, n_map, n, params)) return SEG3D_EINVAL;
    if ((far_idx != nullptr) != (near_idx != nullptr) || (far_idx && !counts) || (!far_idx && !far_flag)) return SEG3D_EINVAL;
    if (!src && n_map > n1 + n2) return SEG3D_EINVAL;
    if (point_bytes == 4)
        far_host<float>(static_cast<const float*>(frame1), n1, static_cast<const float*>(frame2), n2, dim, src, op, n_map,
                        idx, n, *params, sample_range, far_flag, far_idx, near_idx, counts);
    else
        far_host<double>(static_cast<const double*>(frame1), n1, static_cast<const double*>(frame2), n2, dim, src, op, n_map,
                         idx, n, *params, sample_range, far_flag, far_idx, near_idx, counts);
    return SEG3D_OK;
}

size_t seg3d_aug_sample_workspace_bytes(int64_t n) {
    SampleWs w;
    size_t bytes = 0;
    if (!sample_carve(nullptr, n > 0 ? n : 0, &w, &bytes)) return 0;
    return bytes;
}

int seg3d_aug_sample_device(const uint8_t* far_flag, int64_t n, int64_t n_samples, uint64_t seed, int32_t* out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || n > INT32_MAX || n_samples < 0 || n_samples > n) return SEG3D_EINVAL;
    if (n_samples == 0) return SEG3D_OK;
    if (!out || !workspace) return SEG3D_EINVAL;
    SampleWs w;
    size_t need = 0;
    if (!sample_carve(workspace, n, &w, &need)) return SEG3D_ELAUNCH;
    if (workspace_bytes < need) return SEG3D_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const unsigned nb = (unsigned)ceil_div64(n, kThreads), mb = (unsigned)ceil_div64(n_samples, kThreads);
    hipLaunchKernelGGL(select_keys_kernel, dim3(nb), dim3(kThreads), 0, st, far_flag, n, seed, w.k0);
    SEG3D_CHECK_LAUNCH();
    size_t bytes = w.tmp_bytes;
    SEG3D_CHECK_HIP(rocprim::radix_sort_keys(w.tmp, bytes, w.k0, w.k1, (size_t)n, 0u, 64u, st));
    hipLaunchKernelGGL(order_keys_kernel, dim3(mb), dim3(kThreads), 0, st, w.k1, n_samples, seed, w.k0);
    SEG3D_CHECK_LAUNCH();
    bytes = w.tmp_bytes;  // sized for n >= n_samples keys
    SEG3D_CHECK_HIP(rocprim::radix_sort_keys(w.tmp, bytes, w.k0, w.k1, (size_t)n_samples, 0u, 64u, st));
    hipLaunchKernelGGL(key_rows_kernel, dim3(mb), dim3(kThreads), 0, st, w.k1, n_samples, out);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_aug_sample_host(const uint8_t* far_flag, int64_t n, int64_t n_samples, uint64_t seed, int32_t* out) {
    if (n < 0 || n > INT32_MAX || n_samples < 0 || n_samples > n) return SEG3D_EINVAL;
    if (n_samples == 0) return SEG3D_OK;
    if (!out) return SEG3D_EINVAL;
    std::vector<uint64_t> keys((size_t)n);
    for (int64_t i = 0; i < n; ++i) keys[i] = select_key(seed, (uint32_t)i, far_flag ? far_flag[i] != 0 : false);
    std::sort(keys.begin(), keys.end());
    for (int64_t i = 0; i < n_samples; ++i) keys[i] = order_key(seed, (uint32_t)(keys[i] & 0xFFFFFFFFull));
    std::sort(keys.begin(), keys.begin() + n_samples);
    for (int64_t i = 0; i < n_samples; ++i) out[i] = (int32_t)(keys[i] & 0xFFFFFFFFull);
    return SEG3D_OK;
}

size_t seg3d_aug_cur_map_workspace_bytes(int64_t m, int64_t n_points) {
    size_t bytes = 0;
    cur_carve(nullptr, m > 0 ? m : 0, n_points > 0 ? n_points : 0, &bytes);
    return bytes;
}

int seg3d_aug_cur_map(const int32_t* src, int64_t m, const int32_t* cur_point_indices, int64_t n_cur, int64_t n_points,
                      int32_t* cur_pos, int32_t* cur_gather, int32_t* count, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (m < 0 || n_cur < 0 || n_points < 0 || m > INT32_MAX || n_cur > INT32_MAX || n_points > INT32_MAX || !count ||
        !workspace)
        return SEG3D_EINVAL;
    if ((m > 0 && (!src || !cur_pos || !cur_gather)) || (n_cur > 0 && !cur_point_indices)) return SEG3D_EINVAL;
    if (workspace_bytes < seg3d_aug_cur_map_workspace_bytes(m, n_points)) return SEG3D_EWORKSPACE;
    CurWs w = cur_carve(workspace, m, n_points, nullptr);
    hipStream_t st = as_stream(stream);
    SEG3D_CHECK_HIP(hipMemsetAsync(w.inv, 0xFF, ((size_t)n_points + 1) * sizeof(int32_t), st));
    if (n_cur > 0) {
        hipLaunchKernelGGL(cur_scatter_kernel, dim3((unsigned)ceil_div64(n_cur, kThreads)), dim3(kThreads), 0, st,
                           cur_point_indices, n_cur, n_points, w.inv);
        SEG3D_CHECK_LAUNCH();
    }
    const unsigned nb = (unsigned)ceil_div64(m > 0 ? m : 1, kThreads);
    if (m > 0) {
        hipLaunchKernelGGL(cur_flags_kernel, dim3(nb), dim3(kThreads), 0, st, src, m, n_points, w.inv, w.flag);
        SEG3D_CHECK_LAUNCH();
    }
    const int rc = scan_exclusive_u32(w.flag, w.pos, m, w.total, w.tmp, st);
    if (rc != SEG3D_OK) return rc;
    hipLaunchKernelGGL(cur_emit_kernel, dim3(nb), dim3(kThreads), 0, st, src, m, w.inv, w.flag, w.pos, w.total, cur_pos,
                       cur_gather, count);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_aug_cur_map_host(const int32_t* src, int64_t m, const int32_t* cur_point_indices, int64_t n_cur, int64_t n_points,
                           int32_t* cur_pos, int32_t* cur_gather, int32_t* count) {
    if (m < 0 || n_cur < 0 || n_points < 0 || m > INT32_MAX || n_cur > INT32_MAX || n_points > INT32_MAX || !count)
        return SEG3D_EINVAL;
    if ((m > 0 && (!src || !cur_pos || !cur_gather)) || (n_cur > 0 && !cur_point_indices)) return SEG3D_EINVAL;
    std::vector<int32_t> inv((size_t)n_points + 1, -1);
    for (int64_t i = 0; i < n_cur; ++i) {
        const int32_t p = cur_point_indices[i];
        if (p >= 0 && p < n_points) inv[p] = (int32_t)i;
    }
    int32_t o = 0;
    for (int64_t k = 0; k < m; ++k) {
        const int32_t s = src[k];
        if (s >= 0 && s < n_points && inv[s] >= 0) {
            cur_pos[o] = (int32_t)k;
            cur_gather[o++] = inv[s];
        }
    }
    count[0] = o;
    return SEG3D_OK;
}

int seg3d_aug_apply_f32(const float* frame1, int64_t n1, const float* frame2, int64_t n2, int32_t dim, const int32_t* src,
                        const uint8_t* op, int64_t n_out, const seg3d_aug_params* params, float* out, void* stream) {
    return apply_device<float>(frame1, n1, frame2, n2, dim, src, op, n_out, params, out, stream);
}

int seg3d_aug_apply_f64in(const double* frame1, int64_t n1, const double* frame2, int64_t n2, int32_t dim,
                          const int32_t* src, const uint8_t* op, int64_t n_out, const seg3d_aug_params* params, float* out,
                          void* stream) {
    return apply_device<double>(frame1, n1, frame2, n2, dim, src, op, n_out, params, out, stream);
}

int seg3d_aug_apply_host_f32(const float* frame1, int64_t n1, const float* frame2, int64_t n2, int32_t dim,
                             const int32_t* src, const uint8_t* op, int64_t n_out, const seg3d_aug_params* params,
                             float* out) {
    return apply_host<float>(frame1, n1, frame2, n2, dim, src, op, n_out, params, out);
}

int seg3d_aug_apply_host_f64in(const double* frame1, int64_t n1, const double* frame2, int64_t n2, int32_t dim,
                               const int32_t* src, const uint8_t* op, int64_t n_out, const seg3d_aug_params* params,
                               float* out) {
    return apply_host<double>(frame1, n1, frame2, n2, dim, src, op, n_out, params, out);
}

int seg3d_aug_gather(const void* a, int64_t na, const void* b, int64_t nb, int64_t row_bytes, const int32_t* idx, int64_t m,
                     void* out, void* stream) {
    if (!gather_args_ok(a, na, b, nb, row_bytes, idx, m, out)) return SEG3D_EINVAL;
    if (m == 0) return SEG3D_OK;
    hipStream_t st = as_stream(stream);
    const uintptr_t al = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out) |
                         (uintptr_t)row_bytes;
    if ((al & 15) == 0)
        launch_gather<uint4>(a, na, b, nb, row_bytes, idx, m, out, st);
    else if ((al & 7) == 0)
        launch_gather<uint2>(a, na, b, nb, row_bytes, idx, m, out, st);
    else if ((al & 3) == 0)
        launch_gather<uint32_t>(a, na, b, nb, row_bytes, idx, m, out, st);
    else
        launch_gather<uint8_t>(a, na, b, nb, row_bytes, idx, m, out, st);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_aug_gather_host(const void* a, int64_t na, const void* b, int64_t nb, int64_t row_bytes, const int32_t* idx,
                          int64_t m, void* out) {
    if (!gather_args_ok(a, na, b, nb, row_bytes, idx, m, out)) return SEG3D_EINVAL;
    for (int64_t g = 0; g < m; ++g) {
        const int64_t s = idx[g];
        char* o = static_cast<char*>(out) + g * row_bytes;
        if (s >= 0 && s < na)
            memcpy(o, static_cast<const char*>(a) + s * row_bytes, (size_t)row_bytes);
        else if (s >= na && s < na + nb)
            memcpy(o, static_cast<const char*>(b) + (s - na) * row_bytes, (size_t)row_bytes);
        else
            memset(o, 0, (size_t)row_bytes);
    }
    return SEG3D_OK;
}

}  // extern "C"
