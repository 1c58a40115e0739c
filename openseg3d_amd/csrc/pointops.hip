// query_and_group and interpolation of seg3d/utils/pointops_utils.py:25-61 as device ops, forward and backward
// (DESIGN 8i).  The reference gathers through int64 index copies, runs k gather / multiply / add passes for the
// interpolation and takes its gradient through index_put_ float atomics.  Here:
//   forward   grouping: a workgroup takes 256 consecutive (r, i) pairs = one contiguous span of the output; their indices
//             (and the query coordinates) are loaded once, one lane each, into LDS, and the lanes then run over the span's
//             floats element by element -- every store instruction writes 256 contiguous bytes whatever the row length
//             (a 35-float row wastes no lane), every load reads contiguous pieces of source rows.  Four elements per lane
//             are loaded before the first is stored.  With use_xyz = false, c % 4 == 0 and 16-byte aligned pointers the
//             same kernel moves float4 (a row with the 3 coordinates in front is never 16-byte aligned).
//             interpolation: a workgroup takes 1024 / K query rows; index, reciprocal, norm and weight of every slot are
//             computed once per row in LDS (one lane each) and written out for the backward; the lanes then run over the
//             rows' channels (float4 where aligned), four neighbour rows in flight, summing left to right.
//   backward  the store-free half of "store pass + per-destination sum pass": the contribution rows are dout itself, read
//             through the inverse neighbour lists (seg3d_group_index over the flattened idx).  A group of 2..64 lanes per
//             source row (and column tile) walks its list in ascending pair index, four rows in flight.  Lists longer than
//             SEG3D_POINTOPS_CHUNK entries are cut into chunks of that length: the first is summed by the row's own group,
//             every further one by a group of its own into a partial row, and a second small kernel adds the partials to
//             the first chunk's sum in chunk order.  No float atomics; bit-reproducible and bit-equal to the _host twins,
//             which sum in the same order.
// Every index is range-checked before it becomes an address: a slot whose index is outside [0, n) reads nothing.
#include "common.hpp"

#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kPairsPerBlock = 256;  // grouping forward: pairs per workgroup
constexpr int kStage = 1024;         // interpolation forward: (row, slot) entries staged per workgroup
constexpr int kChunk = SEG3D_POINTOPS_CHUNK;
constexpr int kFinishLanes = 8;  // lanes per source row in the pass that adds the partial sums

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int VEC>
struct Row;
template <>
struct Row<1> {
    typedef float T;
    static __host__ __device__ T zero() { return 0.f; }
};
template <>
struct Row<4> {
    typedef f32x4 T;
    static __host__ __device__ T zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
};

__host__ __device__ inline bool row_ok(int32_t j, int64_t n) { return j >= 0 && (int64_t)j < n; }

// ---------------------------------------------------------------------------------------------- grouping forward
// out[p, 0:3] = xyz[idx[p]] - new_xyz[p / K], out[p, 3:] = feat[idx[p]] (p = r * K + i); zeros where idx[p] is outside.
// step_p / step_c: kThreads = step_p * wv + step_c with wv = row length in units of VEC floats (the lanes advance by
// kThreads units per step without dividing).
template <int VEC, bool XYZ>
__global__ __launch_bounds__(kThreads) void group_fwd(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                      const float* __restrict__ feat, const int32_t* __restrict__ idx,
                                                      int64_t n, int64_t pairs, int K, int c, int wv, int step_p,
                                                      int step_c, float* __restrict__ out) {
    typedef typename Row<VEC>::T T;
    __shared__ int32_t s_idx[kPairsPerBlock];
    __shared__ float s_q[XYZ ? kPairsPerBlock * 3 : 1];
    const int64_t p0 = (int64_t)blockIdx.x * kPairsPerBlock;
    const int R = (int)((pairs - p0) < kPairsPerBlock ? (pairs - p0) : kPairsPerBlock);
    const int t = threadIdx.x;
    if (t < R) {
        const int32_t j = idx[p0 + t];
        s_idx[t] = row_ok(j, n) ? j : -1;
        if (XYZ) {
            const int64_t r = (p0 + t) / K;
            s_q[3 * t + 0] = new_xyz[r * 3 + 0];
            s_q[3 * t + 1] = new_xyz[r * 3 + 1];
            s_q[3 * t + 2] = new_xyz[r * 3 + 2];
        }
    }
    __syncthreads();
    const int w = (XYZ ? 3 : 0) + c;  // floats per output row
    int pl = t / wv, col = t % wv;    // pair inside the span, column in units of VEC floats
    while (pl < R) {
        T v[4];
        float q[4];
        int64_t o[4];
        bool live[4], isx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            live[u] = pl < R;
            v[u] = Row<VEC>::zero();
            q[u] = 0.f;
            isx[u] = false;
            o[u] = 0;
            if (live[u]) {
                const int32_t j = s_idx[pl];
                o[u] = (p0 + pl) * (int64_t)w + (int64_t)col * VEC;
                if (j >= 0) {
                    if (XYZ && col < 3) {  // (VEC == 1 whenever XYZ)
                        isx[u] = true;
                        q[u] = s_q[3 * pl + col];
                        v[u] = *reinterpret_cast<const T*>(xyz + (int64_t)j * 3 + col);
                    } else {
                        v[u] = *reinterpret_cast<const T*>(feat + (int64_t)j * c + ((int64_t)col * VEC - (XYZ ? 3 : 0)));
                    }
                }
            }
            col += step_c;
            pl += step_p;
            if (col >= wv) {
                col -= wv;
                ++pl;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!live[u]) continue;
            T r = v[u];
            if (isx[u]) r = r - q[u];  // one float32 subtraction; the feature part is a bit copy
            *reinterpret_cast<T*>(out + o[u]) = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------- interpolation forward
template <int VEC>
__global__ __launch_bounds__(kThreads) void interp_fwd(const float* __restrict__ feat, const int32_t* __restrict__ idx,
                                                       const float* __restrict__ dist, int64_t n, int64_t m, int K, int c,
                                                       int rows_per_block, int cv, int step_p, int step_c,
                                                       float* __restrict__ out, float* __restrict__ w_out) {
    typedef typename Row<VEC>::T T;
    __shared__ int32_t s_idx[kStage];
    __shared__ float s_w[kStage];
    __shared__ float s_norm[kStage];
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int R = (int)((m - r0) < rows_per_block ? (m - r0) : rows_per_block);
    const int E = R * K;
    const int t = threadIdx.x;
    for (int e = t; e < E; e += kThreads) {
        const int32_t j = idx[r0 * K + e];
        s_idx[e] = row_ok(j, n) ? j : -1;
        s_w[e] = 1.0f / (dist[r0 * K + e] + 1e-8f);
    }
    __syncthreads();
    for (int r = t; r < R; r += kThreads) {
        float s = s_w[r * K];
        for (int i = 1; i < K; ++i) s = s + s_w[r * K + i];  // left to right; an outside slot's reciprocal stays in
        s_norm[r] = s;
    }
    __syncthreads();
    for (int e = t; e < E; e += kThreads) {  // (entry e is read and rewritten by the same lane)
        const float wgt = s_w[e] / s_norm[e / K];
        s_w[e] = wgt;
        if (w_out) w_out[r0 * K + e] = wgt;
    }
    __syncthreads();
    int pl = t / cv, col = t % cv;
    while (pl < R) {
        T acc = Row<VEC>::zero();
        const int32_t* ji = s_idx + pl * K;
        const float* wi = s_w + pl * K;
        const float* src = feat + (int64_t)col * VEC;
        for (int i0 = 0; i0 < K; i0 += 4) {
            T v[4];
            float wgt[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t j = (i0 + u < K) ? ji[i0 + u] : -1;
                ok[u] = j >= 0;
                wgt[u] = ok[u] ? wi[i0 + u] : 0.f;
                v[u] = ok[u] ? *reinterpret_cast<const T*>(src + (int64_t)j * c) : Row<VEC>::zero();
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u]) acc = acc + v[u] * wgt[u];  // product and sum rounded separately (-ffp-contract=off)
        }
        *reinterpret_cast<T*>(out + (r0 + pl) * (int64_t)c + (int64_t)col * VEC) = acc;
        col += step_c;
        pl += step_p;
        if (col >= cv) {
            col -= cv;
            ++pl;
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward sums
struct SumArgs {
    const float* dout;      // contribution rows: [pairs, w] (grouping) or [m, w] (interpolation)
    const float* weight;    // [pairs], interpolation only
    const int32_t* idx;     // [pairs]
    const int32_t* order;   // pairs grouped by source row, ascending inside a row
    const int32_t* offsets; // [n + 1]
    int64_t n, nslots;
    int K, w;               // w = floats per contribution row
    int cbeg, ncolv;        // first float column summed, number of VEC-wide columns summed
    int glog2, ntiles;      // lanes per (row, tile) group = 1 << glog2; tiles per row
    int split, c;           // grouping with xyz: columns < split go to d0 (rows of 3), the others to d1 (rows of c)
    float *d0, *d1, *partial;
};

__device__ __forceinline__ float* sum_dest(const SumArgs& a, int64_t j, int col) {
    return col < a.split ? a.d0 + j * 3 + col : a.d1 + j * (int64_t)a.c + (col - a.split);
}

// units 0 .. n * ntiles - 1: source row j, its first chunk, written to the gradient row itself;
// units after them: chunk slot s = (position in pair_order) / kChunk.  A list's further chunks start at offsets[j] +
// q * kChunk (q >= 1); no two of them start in the same slot, and the only candidate in slot s belongs to the row that
// owns position s * kChunk, so every slot finds its chunk (or that it has none) without a table.
template <int VEC, bool INTERP>
__global__ __launch_bounds__(kThreads) void scatter_sum(const SumArgs a) {
    typedef typename Row<VEC>::T T;
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t unit = gid >> a.glog2;
    const int lane = (int)(gid & ((1 << a.glog2) - 1));
    const int64_t uu = unit / a.ntiles;
    const int colv = (int)(unit % a.ntiles) * (1 << a.glog2) + lane;
    if (colv >= a.ncolv) return;
    const int col = a.cbeg + colv * VEC;
    int32_t b, e;
    float* dest;
    if (uu < a.n) {
        b = a.offsets[uu];
        e = a.offsets[uu + 1];
        if (e - b > kChunk) e = b + kChunk;
        dest = sum_dest(a, uu, col);
    } else {
        const int64_t s = uu - a.n;
        if (s >= a.nslots) return;
        const int64_t t0 = s * kChunk;
        if (t0 >= a.offsets[a.n]) return;
        const int32_t pr = a.order[t0];
        const int32_t j = a.idx[pr];
        if (!row_ok(j, a.n)) return;  // (cannot happen for lists built by seg3d_group_index)
        const int32_t bj = a.offsets[j], ej = a.offsets[j + 1];
        const int64_t q = (t0 - bj + kChunk - 1) / kChunk;
        const int64_t st = bj + q * kChunk;
        if (q < 1 || st >= ej) return;
        b = (int32_t)st;
        e = ej - b > kChunk ? b + kChunk : ej;
        dest = a.partial + s * (int64_t)a.w + col;
    }
    T acc = Row<VEC>::zero();
    for (int32_t t = b; t < e; t += 4) {
        T v[4];
        float sc[4];
        bool live[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            live[u] = t + u < e;
            v[u] = Row<VEC>::zero();
            sc[u] = 0.f;
            if (live[u]) {
                const int32_t p = a.order[t + u];
                const int64_t row = INTERP ? (int64_t)((uint32_t)p / (uint32_t)a.K) : (int64_t)p;
                if (INTERP) sc[u] = a.weight[p];
                v[u] = *reinterpret_cast<const T*>(a.dout + row * a.w + col);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (live[u]) acc = INTERP ? acc + v[u] * sc[u] : acc + v[u];
    }
    *reinterpret_cast<T*>(dest) = acc;
}

// rows whose list is longer than a chunk: gradient = ((first chunk + partial 1) + partial 2) + ... in chunk order
__global__ __launch_bounds__(kThreads) void scatter_finish(const SumArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t j = gid / kFinishLanes;
    if (j >= a.n) return;
    const int32_t b = a.offsets[j], e = a.offsets[j + 1];
    if (e - b <= kChunk) return;
    const int ncol = a.ncolv;  // (called with the column count in floats)
    for (int cc = (int)(gid % kFinishLanes); cc < ncol; cc += kFinishLanes) {
        const int col = a.cbeg + cc;
        float* dest = sum_dest(a, j, col);
        float acc = *dest;
        for (int64_t st = (int64_t)b + kChunk; st < e; st += kChunk) acc = acc + a.partial[(st / kChunk) * a.w + col];
        *dest = acc;
    }
}

// dnew_xyz[r] = -((0 + dout[r, 0, 0:3]) + dout[r, 1, 0:3] + ...), slots with an outside index left out
__global__ __launch_bounds__(kThreads) void group_bwd_query(const float* __restrict__ dout, const int32_t* __restrict__ idx,
                                                            int64_t n, int64_t m, int K, int w,
                                                            float* __restrict__ dnew_xyz) {
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (gid >= m * 3) return;
    const int64_t r = gid / 3;
    const int comp = (int)(gid % 3);
    float acc = 0.f;
    for (int i = 0; i < K; ++i)
        if (row_ok(idx[r * K + i], n)) acc = acc + dout[(r * K + i) * w + comp];
    dnew_xyz[gid] = -acc;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool bad_sizes(int64_t n, int64_t m, int32_t k, int32_t c) {
    return n < 0 || m < 0 || k < 1 || k > 64 || c < 1 || (int64_t)c + 3 > 0x7FFFFFFF || m * (int64_t)k >= (int64_t)0x7F000000;
}

// lanes per group: the power of two (at least 32 bytes wide) that pads the row least, the wider one on a tie
void pick_group(int ncolv, int vec, int* glog2, int* ntiles) {
    int best = -1;
    int64_t best_pad = 0;
    for (int lg = (vec == 4 ? 1 : 3); lg <= 6; ++lg) {
        const int64_t g = 1 << lg, pad = ((int64_t)ncolv + g - 1) / g * g;
        if (best < 0 || pad <= best_pad) best = lg, best_pad = pad;
    }
    *glog2 = best;
    *ntiles = (int)(((int64_t)ncolv + (1 << best) - 1) >> best);
}

template <bool INTERP>
int launch_sums(SumArgs a, bool vec4, hipStream_t st) {
    const int vec = vec4 ? 4 : 1;
    const int ncol = a.ncolv;  // floats on entry
    a.ncolv = ncol / vec;
    pick_group(a.ncolv, vec, &a.glog2, &a.ntiles);
    const int64_t threads = ((a.n + a.nslots) * a.ntiles) << a.glog2;
    const int64_t blocks = ceil_div64(threads, kThreads);
    if (blocks >= 0x7FFFFFFF) return SEG3D_EINVAL;
    if (vec4)
        hipLaunchKernelGGL((scatter_sum<4, INTERP>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL((scatter_sum<1, INTERP>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    SEG3D_CHECK_LAUNCH();
    a.ncolv = ncol;
    hipLaunchKernelGGL(scatter_finish, dim3((unsigned)ceil_div64(a.n * kFinishLanes, kThreads)), dim3(kThreads), 0, st, a);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

// ---------------------------------------------------------------------------------------------- host twins' sum
// the same order as the kernels: chunks of kChunk entries, each summed from 0, added in chunk order
template <typename Term>
void host_list_sum(const int32_t* order, int32_t b, int32_t e, int ncol, float* dest, std::vector<float>& part, Term term) {
    int32_t cb = b;
    do {
        const int32_t ce = e - cb > kChunk ? cb + kChunk : e;
        float* acc = cb == b ? dest : part.data();
        for (int col = 0; col < ncol; ++col) acc[col] = 0.f;
        for (int32_t t = cb; t < ce; ++t)
            for (int col = 0; col < ncol; ++col) acc[col] = acc[col] + term(order[t], col);
        if (cb != b)
            for (int col = 0; col < ncol; ++col) dest[col] = dest[col] + acc[col];
        cb = ce;
    } while (cb < e);
}

}  // namespace

extern "C" {

size_t seg3d_pointops_scratch_bytes(int64_t m, int32_t k, int32_t width) {
    if (m < 0 || k < 1 || width < 1) return 0;
    const int64_t slots = ceil_div64(m * (int64_t)k, kChunk);
    return align_up((size_t)(slots > 0 ? slots : 1) * (size_t)width * sizeof(float), 256);
}

int seg3d_group_points_fwd(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, int64_t n,
                           int64_t m, int32_t k, int32_t c, float* out, void* stream) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0) return SEG3D_OK;
    if (!feat || !idx || !out || (xyz && !new_xyz)) return SEG3D_EINVAL;
    const int64_t pairs = m * k;
    const unsigned blocks = (unsigned)ceil_div64(pairs, kPairsPerBlock);
    hipStream_t st = as_stream(stream);
    if (xyz) {
        const int wv = c + 3;
        hipLaunchKernelGGL((group_fwd<1, true>), dim3(blocks), dim3(kThreads), 0, st, xyz, new_xyz, feat, idx, n, pairs,
                           k, c, wv, kThreads / wv, kThreads % wv, out);
    } else if (c % 4 == 0 && aligned16(feat) && aligned16(out)) {
        const int wv = c / 4;
        hipLaunchKernelGGL((group_fwd<4, false>), dim3(blocks), dim3(kThreads), 0, st, xyz, new_xyz, feat, idx, n, pairs,
                           k, c, wv, kThreads / wv, kThreads % wv, out);
    } else {
        hipLaunchKernelGGL((group_fwd<1, false>), dim3(blocks), dim3(kThreads), 0, st, xyz, new_xyz, feat, idx, n, pairs,
                           k, c, c, kThreads / c, kThreads % c, out);
    }
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_group_points_fwd_host(const float* xyz, const float* new_xyz, const float* feat, const int32_t* idx, int64_t n,
                                int64_t m, int32_t k, int32_t c, float* out) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0) return SEG3D_OK;
    if (!feat || !idx || !out || (xyz && !new_xyz)) return SEG3D_EINVAL;
    const int64_t w = (xyz ? 3 : 0) + (int64_t)c;
    for (int64_t p = 0; p < m * k; ++p) {
        float* o = out + p * w;
        const int32_t j = idx[p];
        if (!row_ok(j, n)) {
            for (int64_t col = 0; col < w; ++col) o[col] = 0.f;
            continue;
        }
        if (xyz) {
            const float* q = new_xyz + (p / k) * 3;
            for (int d = 0; d < 3; ++d) o[d] = xyz[(int64_t)j * 3 + d] - q[d];
            o += 3;
        }
        for (int32_t col = 0; col < c; ++col) o[col] = feat[(int64_t)j * c + col];
    }
    return SEG3D_OK;
}

int seg3d_group_points_bwd(const float* dout, const int32_t* idx, const int32_t* pair_order, const int32_t* pair_offsets,
                           int64_t n, int64_t m, int32_t k, int32_t c, int32_t with_xyz, float* dxyz, float* dnew_xyz,
                           float* dfeat, void* scratch, size_t scratch_bytes, void* stream) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0) return SEG3D_OK;
    if (!with_xyz && (dxyz || dnew_xyz)) return SEG3D_EINVAL;
    if (!dxyz && !dnew_xyz && !dfeat) return SEG3D_OK;
    if (!dout || !idx) return SEG3D_EINVAL;
    hipStream_t st = as_stream(stream);
    const int w = (with_xyz ? 3 : 0) + c;
    if (dnew_xyz) {
        hipLaunchKernelGGL(group_bwd_query, dim3((unsigned)ceil_div64(m * 3, kThreads)), dim3(kThreads), 0, st, dout, idx,
                           n, m, k, w, dnew_xyz);
        SEG3D_CHECK_LAUNCH();
    }
    if (!dxyz && !dfeat) return SEG3D_OK;
    if (!pair_order || !pair_offsets || !scratch) return SEG3D_EINVAL;
    if (scratch_bytes < seg3d_pointops_scratch_bytes(m, k, w)) return SEG3D_EWORKSPACE;
    SumArgs a;
    a.dout = dout;
    a.weight = nullptr;
    a.idx = idx;
    a.order = pair_order;
    a.offsets = pair_offsets;
    a.n = n;
    a.nslots = ceil_div64(m * (int64_t)k, kChunk);
    a.K = k;
    a.w = w;
    a.split = with_xyz ? 3 : 0;
    a.c = c;
    a.d0 = dxyz;
    a.d1 = dfeat;
    a.partial = static_cast<float*>(scratch);
    a.cbeg = dxyz ? 0 : a.split;            // one launch sums the coordinate and the feature columns together;
    a.ncolv = (dfeat ? w : a.split) - a.cbeg;  // columns nobody asked for are not read
    const bool vec4 = !with_xyz && c % 4 == 0 && aligned16(dout) && aligned16(dfeat) && aligned16(scratch);
    return launch_sums<false>(a, vec4, st);
}

int seg3d_group_points_bwd_host(const float* dout, const int32_t* idx, const int32_t* pair_order,
                                const int32_t* pair_offsets, int64_t n, int64_t m, int32_t k, int32_t c,
                                int32_t with_xyz, float* dxyz, float* dnew_xyz, float* dfeat) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0) return SEG3D_OK;
    if (!with_xyz && (dxyz || dnew_xyz)) return SEG3D_EINVAL;
    if (!dxyz && !dnew_xyz && !dfeat) return SEG3D_OK;
    if (!dout || !idx) return SEG3D_EINVAL;
    const int64_t w = (with_xyz ? 3 : 0) + (int64_t)c;
    if (dnew_xyz) {
        for (int64_t r = 0; r < m; ++r)
            for (int d = 0; d < 3; ++d) {
                float acc = 0.f;
                for (int i = 0; i < k; ++i)
                    if (row_ok(idx[r * k + i], n)) acc = acc + dout[(r * k + i) * w + d];
                dnew_xyz[r * 3 + d] = -acc;
            }
    }
    if (!dxyz && !dfeat) return SEG3D_OK;
    if (!pair_order || !pair_offsets) return SEG3D_EINVAL;
    std::vector<float> part((size_t)w), row((size_t)w);
    const int split = with_xyz ? 3 : 0;
    for (int64_t j = 0; j < n; ++j) {
        host_list_sum(pair_order, pair_offsets[j], pair_offsets[j + 1], (int)w, row.data(), part,
                      [&](int32_t p, int col) { return dout[(int64_t)p * w + col]; });
        if (dxyz)
            for (int d = 0; d < 3; ++d) dxyz[j * 3 + d] = row[d];
        if (dfeat)
            for (int32_t col = 0; col < c; ++col) dfeat[j * c + col] = row[split + col];
    }
    return SEG3D_OK;
}

int seg3d_knn_interpolate_fwd(const float* feat, const int32_t* idx, const float* dist, int64_t n, int64_t m, int32_t k,
                              int32_t c, float* out, float* weight, void* stream) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0) return SEG3D_OK;
    if (!feat || !idx || !dist || !out) return SEG3D_EINVAL;
    const int rows = kStage / k;
    const unsigned blocks = (unsigned)ceil_div64(m, rows);
    hipStream_t st = as_stream(stream);
    if (c % 4 == 0 && aligned16(feat) && aligned16(out)) {
        const int cv = c / 4;
        hipLaunchKernelGGL(interp_fwd<4>, dim3(blocks), dim3(kThreads), 0, st, feat, idx, dist, n, m, k, c, rows, cv,
                           kThreads / cv, kThreads % cv, out, weight);
    } else {
        hipLaunchKernelGGL(interp_fwd<1>, dim3(blocks), dim3(kThreads), 0, st, feat, idx, dist, n, m, k, c, rows, c,
                           kThreads / c, kThreads % c, out, weight);
    }
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_knn_interpolate_fwd_host(const float* feat, const int32_t* idx, const float* dist, int64_t n, int64_t m,
                                   int32_t k, int32_t c, float* out, float* weight) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0) return SEG3D_OK;
    if (!feat || !idx || !dist || !out) return SEG3D_EINVAL;
    float wgt[64];
    for (int64_t r = 0; r < m; ++r) {
        for (int i = 0; i < k; ++i) wgt[i] = 1.0f / (dist[r * k + i] + 1e-8f);
        float norm = wgt[0];
        for (int i = 1; i < k; ++i) norm = norm + wgt[i];
        for (int i = 0; i < k; ++i) {
            wgt[i] = wgt[i] / norm;
            if (weight) weight[r * k + i] = wgt[i];
        }
        float* o = out + r * c;
        for (int32_t col = 0; col < c; ++col) o[col] = 0.f;
        for (int i = 0; i < k; ++i) {
            const int32_t j = idx[r * k + i];
            if (!row_ok(j, n)) continue;
            const float* src = feat + (int64_t)j * c;
            for (int32_t col = 0; col < c; ++col) o[col] = o[col] + src[col] * wgt[i];
        }
    }
    return SEG3D_OK;
}

int seg3d_knn_interpolate_bwd(const float* dout, const float* weight, const int32_t* idx, const int32_t* pair_order,
                              const int32_t* pair_offsets, int64_t n, int64_t m, int32_t k, int32_t c, float* dfeat,
                              void* scratch, size_t scratch_bytes, void* stream) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0 || !dfeat) return SEG3D_OK;
    if (!dout || !weight || !idx || !pair_order || !pair_offsets || !scratch) return SEG3D_EINVAL;
    if (scratch_bytes < seg3d_pointops_scratch_bytes(m, k, c)) return SEG3D_EWORKSPACE;
    SumArgs a;
    a.dout = dout;
    a.weight = weight;
    a.idx = idx;
    a.order = pair_order;
    a.offsets = pair_offsets;
    a.n = n;
    a.nslots = ceil_div64(m * (int64_t)k, kChunk);
    a.K = k;
    a.w = c;
    a.split = 0;
    a.c = c;
    a.d0 = nullptr;
    a.d1 = dfeat;
    a.partial = static_cast<float*>(scratch);
    a.cbeg = 0;
    a.ncolv = c;
    const bool vec4 = c % 4 == 0 && aligned16(dout) && aligned16(dfeat) && aligned16(scratch);
    return launch_sums<true>(a, vec4, as_stream(stream));
}

int seg3d_knn_interpolate_bwd_host(const float* dout, const float* weight, const int32_t* idx, const int32_t* pair_order,
                                   const int32_t* pair_offsets, int64_t n, int64_t m, int32_t k, int32_t c,
                                   float* dfeat) {
    if (bad_sizes(n, m, k, c)) return SEG3D_EINVAL;
    if (m == 0 || n == 0 || !dfeat) return SEG3D_OK;
    if (!dout || !weight || !idx || !pair_order || !pair_offsets) return SEG3D_EINVAL;
    std::vector<float> part((size_t)c);
    for (int64_t j = 0; j < n; ++j)
        host_list_sum(pair_order, pair_offsets[j], pair_offsets[j + 1], c, dfeat + j * c, part,
                      [&](int32_t p, int col) { return dout[(int64_t)(p / k) * c + col] * weight[p]; });
    return SEG3D_OK;
}

}  // extern "C"
