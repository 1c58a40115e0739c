// One-output-channel submanifold convolution with an optional fused sigmoid gate: SALayer of
// seg3d/models/layers/sa_layer.py:8-25 (SubMConv3d(planes, 1, 3, padding=1, bias=False) -> sigmoid -> x * gate) and the
// plain C -> 1 conv behind it.  The contract, summation orders included, is in include/seg3d_hip.h.
//   forward   a gather-dot.  A row is handled by a group of L = 1..64 lanes (the power of two >= C / 4, at most 64), every
//             lane loading 16-byte pieces of the gathered rows.  The workgroup first stages the weight (up to 48 KB) and
//             its rows' slice of the table in LDS; a lane then requests all present neighbour rows of a pass before it
//             consumes the first (a gather-latency kernel: one round trip per pass), offsets without a neighbour load
//             nothing.  Rows longer than 256 floats take 2 or 4 passes.  One butterfly per row, then the logit and --
//             fused -- y = x * sigmoid(s) from the centre row already in registers.
//   ds        the row dot dy . x with the same lane layout, times the sigmoid's slope.
//   backward  by the table's mirror property (nbr[k][i] == j  <=>  nbr[26 - k][j] == i) both gradients of row j need only
//             the 27 scalars d[k] = ds[nbr[k][j]]:  dx_j = dy_j g_j + sum_k d[k] w[26 - k],  dw[26 - k] += d[k] x_j.
//             A workgroup takes SEG3D_SUBM_DOT_ROWS consecutive rows, stages their 27 scalars (and gates) in LDS, and
//             every lane owns one channel: it keeps 27 weights and 27 weight-gradient accumulators in registers while the
//             block's rows stream past once (x and dy read once, four rows in flight, dx written once, coalesced).  The block's partial
//             weight gradient goes to scratch; a second small kernel adds the partials in block order.  No float atomics.
// The _host twins are plain C++ in the same order of operations: same bits wherever no expf is involved.
#include "common.hpp"

#include <math.h>

#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kRows = SEG3D_SUBM_DOT_ROWS;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// lanes per row: the power of two >= C / 4, at most 64
inline int lanes_for(int c) {
    int l = 1;
    while (l < c / 4 && l < 64) l <<= 1;
    return l;
}

__host__ __device__ inline float dot4(f32x4 a, f32x4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

// overflow-safe: expf of a non-positive number only
__host__ __device__ inline float sigmoid_f(float s) {
    const float e = expf(-fabsf(s));
    return s >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

__host__ __device__ inline float sigmoid_slope(float dg, float g) { return (dg * g) * (1.0f - g); }

template <int L>
__device__ __forceinline__ float group_tree(float q) {
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) q = q + __shfl_xor(q, off, 64);
    return q;
}

// ---------------------------------------------------------------------------------------------- forward
// P = passes of L lanes over a row (P > 1 only with L == 64).  Dynamic LDS: the weight [27][C] when WLDS (it fits), then
// the workgroup's slice of the table as [row][28] (27 offsets + a pad), so that a lane reads its row's offsets as seven
// 16-byte LDS loads instead of 27 global ones.
constexpr int kIdxStride = 28;

template <int L, int P, bool WLDS>
__global__ __launch_bounds__(kThreads) void subm_dot_fwd(const float* __restrict__ x, const int32_t* __restrict__ nbr,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         int64_t M, int C, float* __restrict__ s_out,
                                                         float* __restrict__ y_out) {
    constexpr int kRowsPerBlock = kThreads / L;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nv = C / 4;
    f32x4* s_w = reinterpret_cast<f32x4*>(smem);
    int32_t* s_idx = reinterpret_cast<int32_t*>(smem + (WLDS ? (size_t)27 * C * sizeof(float) : 0));
    const int64_t row0 = (int64_t)blockIdx.x * kRowsPerBlock;
    if (WLDS)
        for (int e = threadIdx.x; e < 27 * nv; e += kThreads) s_w[e] = reinterpret_cast<const f32x4*>(w)[e];
    for (int e = threadIdx.x; e < 27 * kRowsPerBlock; e += kThreads) {
        const int k = e / kRowsPerBlock, r = e % kRowsPerBlock;
        const int32_t v = row0 + r < M ? nbr[(int64_t)k * M + row0 + r] : -1;
        s_idx[r * kIdxStride + k] = (v >= 0 && (int64_t)v < M) ? v : -1;  // never an address unless it is a row of x
        if (k == 0) s_idx[r * kIdxStride + 27] = -1;
    }
    __syncthreads();
    const int l = threadIdx.x % L;
    const int rl = threadIdx.x / L;
    const int64_t i = row0 + rl;
    const bool row = i < M;
    int32_t n[kIdxStride];
#pragma unroll
    for (int k4 = 0; k4 < kIdxStride / 4; ++k4) {
        const int4 v = *reinterpret_cast<const int4*>(s_idx + rl * kIdxStride + k4 * 4);
        n[k4 * 4 + 0] = v.x;
        n[k4 * 4 + 1] = v.y;
        n[k4 * 4 + 2] = v.z;
        n[k4 * 4 + 3] = v.w;
    }
    float q = 0.f;
    f32x4 centre[P];
#pragma unroll
    for (int t = 0; t < P; ++t) {
        const int c4 = l + t * L;
        const bool col = c4 < nv;
        centre[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float a = 0.f;
        // every present neighbour row is requested before the first is consumed: one round trip per pass
        f32x4 xv[27];
#pragma unroll
        for (int k = 0; k < 27; ++k)
            if (col && n[k] >= 0) xv[k] = *reinterpret_cast<const f32x4*>(x + (int64_t)n[k] * C + c4 * 4);
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            if (col && n[k] >= 0) {
                const f32x4 wv = WLDS ? s_w[k * nv + c4] : *reinterpret_cast<const f32x4*>(w + k * C + c4 * 4);
                a = a + dot4(xv[k], wv);
                if (k == 13) centre[t] = xv[k];
            }
        }
        if (col) q = t == 0 ? a : q + a;
    }
    q = group_tree<L>(q);
    if (!row) return;
    const float s = bias ? q + bias[0] : q;
    if (l == 0) s_out[i] = s;
    if (y_out) {
        const float g = sigmoid_f(s);
#pragma unroll
        for (int t = 0; t < P; ++t) {
            const int c4 = l + t * L;
            if (c4 < nv) *reinterpret_cast<f32x4*>(y_out + i * C + c4 * 4) = centre[t] * g;
        }
    }
}

// ---------------------------------------------------------------------------------------------- ds = (dy . x) g (1 - g)
template <int L, int P>
__global__ __launch_bounds__(kThreads) void subm_dot_ds(const float* __restrict__ dy, const float* __restrict__ x,
                                                        const float* __restrict__ s, int64_t M, int C,
                                                        float* __restrict__ ds) {
    constexpr int kRowsPerBlock = kThreads / L;
    const int l = threadIdx.x % L;
    const int64_t i = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / L;
    const bool row = i < M;
    const int nv = C / 4;
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < P; ++t) {
        const int c4 = l + t * L;
        if (row && c4 < nv) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(dy + i * C + c4 * 4);
            const f32x4 b = *reinterpret_cast<const f32x4*>(x + i * C + c4 * 4);
            const float p = 0.f + dot4(a, b);
            q = t == 0 ? p : q + p;
        }
    }
    q = group_tree<L>(q);
    if (row && l == 0) ds[i] = sigmoid_slope(q, sigmoid_f(s[i]));
}

// ---------------------------------------------------------------------------------------------- backward
// One workgroup per block of kRows rows and 256 channels; lane = channel.
constexpr int kBwdInFlight = 4;

template <bool DY, bool DX, bool DW>
__global__ __launch_bounds__(kThreads) void subm_dot_bwd(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ s, const float* __restrict__ ds,
                                                         const int32_t* __restrict__ nbr, const float* __restrict__ w,
                                                         int64_t M, int C, float* __restrict__ dx,
                                                         float* __restrict__ part_dw, float* __restrict__ part_db) {
    // per row the 27 scalars d[k] = ds[nbr[k][r]] (0 where the offset has no neighbour) and a pad: seven 16-byte reads
    __shared__ __attribute__((aligned(16))) float s_d[kRows * kIdxStride];
    __shared__ float s_g[kRows];
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    const int R = (int)((M - r0) < kRows ? (M - r0) : kRows);
    const int t = threadIdx.x;
    for (int r = t; r < R; r += blockDim.x) {
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const int32_t j = nbr[(int64_t)k * M + r0 + r];
            s_d[r * kIdxStride + k] = (j >= 0 && (int64_t)j < M) ? ds[j] : 0.f;
        }
        s_d[r * kIdxStride + 27] = 0.f;
        if (DY) s_g[r] = sigmoid_f(s[r0 + r]);
    }
    __syncthreads();
    const int c = blockIdx.y * blockDim.x + t;
    if (c < C) {
        float wr[27], acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            wr[k] = DX ? w[(26 - k) * C + c] : 0.f;  // wr[k] multiplies d[k]
            acc[k] = 0.f;
        }
        // one row: no branch inside, so that the next row's LDS reads are scheduled over this row's arithmetic
        auto step = [&](int r, float xv, float dyv) {
            float d[kIdxStride];
#pragma unroll
            for (int k4 = 0; k4 < kIdxStride / 4; ++k4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(s_d + r * kIdxStride + k4 * 4);
                d[k4 * 4 + 0] = v.x;
                d[k4 * 4 + 1] = v.y;
                d[k4 * 4 + 2] = v.z;
                d[k4 * 4 + 3] = v.w;
            }
            float tsum = 0.f;
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                if (DX) tsum = tsum + d[k] * wr[k];
                if (DW) acc[k] = acc[k] + d[k] * xv;
            }
            if (DX) dx[(r0 + r) * C + c] = DY ? dyv * s_g[r] + tsum : tsum;
        };
        int rb = 0;
        for (; rb + kBwdInFlight <= R; rb += kBwdInFlight) {  // kBwdInFlight rows of x and dy are loaded before the first is used
            float xv[kBwdInFlight], dyv[kBwdInFlight];
#pragma unroll
            for (int u = 0; u < kBwdInFlight; ++u) {
                const int64_t o = (r0 + rb + u) * C + c;
                xv[u] = DW ? x[o] : 0.f;
                dyv[u] = (DY && DX) ? dy[o] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kBwdInFlight; ++u) step(rb + u, xv[u], dyv[u]);
        }
        for (; rb < R; ++rb) {
            const int64_t o = (r0 + rb) * C + c;
            step(rb, DW ? x[o] : 0.f, (DY && DX) ? dy[o] : 0.f);
        }
        if (DW) {
            float* out = part_dw + (int64_t)blockIdx.x * 27 * C;
#pragma unroll
            for (int k = 0; k < 27; ++k) out[(26 - k) * C + c] = acc[k];  // d[k] belongs to dw[26 - k]
        }
    }
    if (DW && part_db && blockIdx.y == 0 && t == 0) {
        float b = 0.f;
        for (int r = 0; r < R; ++r) b = b + s_d[r * kIdxStride + 13];  // d[13] of row r is ds[r]
        part_db[blockIdx.x] = b;
    }
}

// dw[e] = ((0 + part[0][e]) + part[1][e]) + ...; the thread after the last element does the same for dbias.  The chain of
// additions is fixed, the loads are not part of it: kFoldInFlight partials are requested before the first is added.
constexpr int kFoldInFlight = 32;

__device__ __forceinline__ float fold_chain(const float* __restrict__ part, int64_t blocks, int64_t stride) {
    float v = 0.f;
    for (int64_t b0 = 0; b0 < blocks; b0 += kFoldInFlight) {
        float p[kFoldInFlight];
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) p[u] = b0 + u < blocks ? part[(b0 + u) * stride] : 0.f;
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u)
            if (b0 + u < blocks) v = v + p[u];
    }
    return v;
}

__global__ __launch_bounds__(kThreads) void subm_dot_fold(const float* __restrict__ part_dw,
                                                          const float* __restrict__ part_db, int64_t blocks, int E,
                                                          float* __restrict__ dw, float* __restrict__ dbias) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e < E && dw) dw[e] = fold_chain(part_dw + e, blocks, E);
    if (e == E && dbias) dbias[0] = fold_chain(part_db, blocks, 1);
}

inline bool shape_ok(int64_t M, int32_t C) { return M >= 0 && M < 0x7FFFFFFF && C >= 4 && C <= 1024 && C % 4 == 0; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int64_t row_blocks(int64_t M) { return ceil_div64(M, kRows); }

constexpr size_t kWeightLdsMax = 48 * 1024;  // a [27][C] weight up to this size is staged in LDS (C <= 444)

template <int L, int P>
void launch_fwd(const float* x, const int32_t* nbr, const float* w, const float* bias, int64_t M, int C, float* s_out,
                float* y_out, hipStream_t st) {
    const int64_t grid = ceil_div64(M, kThreads / L);
    const size_t idx_bytes = (size_t)(kThreads / L) * kIdxStride * sizeof(int32_t), w_bytes = (size_t)27 * C * sizeof(float);
    if (w_bytes <= kWeightLdsMax)
        hipLaunchKernelGGL((subm_dot_fwd<L, P, true>), dim3((unsigned)grid), dim3(kThreads), w_bytes + idx_bytes, st, x, nbr,
                           w, bias, M, C, s_out, y_out);
    else
        hipLaunchKernelGGL((subm_dot_fwd<L, P, false>), dim3((unsigned)grid), dim3(kThreads), idx_bytes, st, x, nbr, w, bias,
                           M, C, s_out, y_out);
}

template <int L, int P>
void launch_ds(const float* dy, const float* x, const float* s, int64_t M, int C, float* ds, hipStream_t st) {
    const int64_t grid = ceil_div64(M, kThreads / L);
    hipLaunchKernelGGL((subm_dot_ds<L, P>), dim3((unsigned)grid), dim3(kThreads), 0, st, dy, x, s, M, C, ds);
}

// calls F<L, P>(args...) for the lane layout of C
#define SUBM_DOT_DISPATCH(F, C, ...)                       \
    do {                                                   \
        const int L_ = lanes_for(C);                       \
        const int nv_ = (C) / 4;                           \
        if (L_ == 1) F<1, 1>(__VA_ARGS__);                 \
        else if (L_ == 2) F<2, 1>(__VA_ARGS__);            \
        else if (L_ == 4) F<4, 1>(__VA_ARGS__);            \
        else if (L_ == 8) F<8, 1>(__VA_ARGS__);            \
        else if (L_ == 16) F<16, 1>(__VA_ARGS__);          \
        else if (L_ == 32) F<32, 1>(__VA_ARGS__);          \
        else if (nv_ <= 64) F<64, 1>(__VA_ARGS__);         \
        else if (nv_ <= 128) F<64, 2>(__VA_ARGS__);        \
        else F<64, 4>(__VA_ARGS__);                        \
    } while (0)

template <bool DY, bool DX, bool DW>
void launch_bwd(const float* dy, const float* x, const float* s, const float* ds, const int32_t* nbr, const float* w,
                int64_t M, int C, float* dx, float* part_dw, float* part_db, hipStream_t st) {
    const int threads = C >= kThreads ? kThreads : (C <= 128 ? 128 : kThreads);  // lane = channel; >= 128 lanes stage the block
    const dim3 grid((unsigned)row_blocks(M), (unsigned)((C + threads - 1) / threads));
    hipLaunchKernelGGL((subm_dot_bwd<DY, DX, DW>), grid, dim3(threads), 0, st, dy, x, s, ds, nbr, w, M, C, dx, part_dw,
                       part_db);
}

// the channel reduction of the contract on the host: q[l] per lane, passes in ascending order, then the tree
struct HostTree {
    int L, nv;
    std::vector<float> q;
    explicit HostTree(int C) : L(lanes_for(C)), nv(C / 4), q(lanes_for(C)) {}
    // group(c4) -> the group's value
    template <typename G>
    float run(G group) {
        for (int l = 0; l < L; ++l) {
            float v = 0.f;
            int t = 0;
            for (int c4 = l; c4 < nv; c4 += L, ++t) {
                const float a = group(c4);
                v = t == 0 ? a : v + a;
            }
            q[l] = v;
        }
        for (int off = L / 2; off >= 1; off >>= 1)
            for (int l = 0; l < off; ++l) q[l] = q[l] + q[l + off];
        return q[0];
    }
};

inline f32x4 load4(const float* p) { return (f32x4){p[0], p[1], p[2], p[3]}; }

}  // namespace

extern "C" {

size_t seg3d_subm_dot_scratch_bytes(int64_t M, int32_t C) {
    if (!shape_ok(M, C)) return 0;
    return align_up((size_t)row_blocks(M) * 27 * (size_t)C * sizeof(float), 256) +
           align_up((size_t)row_blocks(M) * sizeof(float), 256);
}

int seg3d_subm_dot_fwd(const float* x, const int32_t* nbr, const float* w, const float* bias, int64_t M, int32_t C,
                       float* s_out, float* y_out, void* stream) {
    if (!shape_ok(M, C)) return SEG3D_EINVAL;
    if (M == 0) return SEG3D_OK;
    if (!x || !nbr || !w || !s_out || !aligned16(x) || !aligned16(w) || !aligned16(y_out)) return SEG3D_EINVAL;
    SUBM_DOT_DISPATCH(launch_fwd, C, x, nbr, w, bias, M, C, s_out, y_out, as_stream(stream));
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_subm_dot_bwd_ds(const float* dy, const float* x, const float* s, int64_t M, int32_t C, float* ds_out,
                          void* stream) {
    if (!shape_ok(M, C)) return SEG3D_EINVAL;
    if (M == 0) return SEG3D_OK;
    if (!dy || !x || !s || !ds_out || !aligned16(dy) || !aligned16(x)) return SEG3D_EINVAL;
    SUBM_DOT_DISPATCH(launch_ds, C, dy, x, s, M, C, ds_out, as_stream(stream));
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_subm_dot_bwd(const float* dy, const float* x, const float* s, const float* ds, const int32_t* nbr,
                       const float* w, int64_t M, int32_t C, float* dx, float* dw, float* dbias, void* scratch,
                       size_t scratch_bytes, void* stream) {
    if (!shape_ok(M, C)) return SEG3D_EINVAL;
    const bool want_w = dw || dbias;
    if (!dx && !want_w) return SEG3D_OK;
    if (M > 0 && (!ds || !nbr || (dy && !s) || (dx && !w) || (want_w && !x))) return SEG3D_EINVAL;
    if (want_w && M > 0 && (!scratch || scratch_bytes < seg3d_subm_dot_scratch_bytes(M, C))) return SEG3D_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const int64_t nb = row_blocks(M);
    float* part_dw = nullptr;
    float* part_db = nullptr;
    if (want_w && M > 0) {
        WsCarver ws(scratch);
        part_dw = ws.take<float>((size_t)nb * 27 * C);
        part_db = ws.take<float>((size_t)nb);
    }
    if (M > 0) {
        const bool DY = dy != nullptr, DX = dx != nullptr;
        if (DY && DX && want_w) launch_bwd<true, true, true>(dy, x, s, ds, nbr, w, M, C, dx, part_dw, part_db, st);
        else if (DY && DX) launch_bwd<true, true, false>(dy, x, s, ds, nbr, w, M, C, dx, part_dw, part_db, st);
        else if (DX && want_w) launch_bwd<false, true, true>(dy, x, s, ds, nbr, w, M, C, dx, part_dw, part_db, st);
        else if (DX) launch_bwd<false, true, false>(dy, x, s, ds, nbr, w, M, C, dx, part_dw, part_db, st);
        else launch_bwd<false, false, true>(dy, x, s, ds, nbr, w, M, C, dx, part_dw, part_db, st);
        SEG3D_CHECK_LAUNCH();
    }
    if (want_w) {
        const int E = 27 * C;
        hipLaunchKernelGGL(subm_dot_fold, dim3((unsigned)((E + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           part_dw, part_db, nb, E, dw, dbias);
        SEG3D_CHECK_LAUNCH();
    }
    return SEG3D_OK;
}

// ---------------------------------------------------------------------------------------------- host twins
int seg3d_subm_dot_fwd_host(const float* x, const int32_t* nbr, const float* w, const float* bias, int64_t M, int32_t C,
                            float* s_out, float* y_out) {
    if (!shape_ok(M, C)) return SEG3D_EINVAL;
    if (M == 0) return SEG3D_OK;
    if (!x || !nbr || !w || !s_out || !aligned16(x) || !aligned16(w) || !aligned16(y_out)) return SEG3D_EINVAL;
    HostTree tree(C);
    for (int64_t i = 0; i < M; ++i) {
        const float q = tree.run([&](int c4) {
            float a = 0.f;
            for (int k = 0; k < 27; ++k) {
                const int32_t j = nbr[(int64_t)k * M + i];
                if (j < 0 || (int64_t)j >= M) continue;
                a = a + dot4(load4(x + (int64_t)j * C + c4 * 4), load4(w + k * C + c4 * 4));
            }
            return a;
        });
        const float s = bias ? q + bias[0] : q;
        s_out[i] = s;
        if (y_out) {
            const int32_t jc = nbr[(int64_t)13 * M + i];
            const bool centre = jc >= 0 && (int64_t)jc < M;
            const float g = sigmoid_f(s);
            for (int c = 0; c < C; ++c) y_out[i * C + c] = (centre ? x[(int64_t)jc * C + c] : 0.f) * g;
        }
    }
    return SEG3D_OK;
}

int seg3d_subm_dot_bwd_ds_host(const float* dy, const float* x, const float* s, int64_t M, int32_t C, float* ds_out) {
    if (!shape_ok(M, C)) return SEG3D_EINVAL;
    if (M == 0) return SEG3D_OK;
    if (!dy || !x || !s || !ds_out || !aligned16(dy) || !aligned16(x)) return SEG3D_EINVAL;
    HostTree tree(C);
    for (int64_t i = 0; i < M; ++i) {
        const float q = tree.run([&](int c4) { return 0.f + dot4(load4(dy + i * C + c4 * 4), load4(x + i * C + c4 * 4)); });
        ds_out[i] = sigmoid_slope(q, sigmoid_f(s[i]));
    }
    return SEG3D_OK;
}

int seg3d_subm_dot_bwd_host(const float* dy, const float* x, const float* s, const float* ds, const int32_t* nbr,
                            const float* w, int64_t M, int32_t C, float* dx, float* dw, float* dbias) {
    if (!shape_ok(M, C)) return SEG3D_EINVAL;
    const bool want_w = dw || dbias;
    if (!dx && !want_w) return SEG3D_OK;
    if (M > 0 && (!ds || !nbr || (dy && !s) || (dx && !w) || (want_w && !x))) return SEG3D_EINVAL;
    const int E = 27 * C;
    std::vector<float> total(want_w ? E : 0, 0.f), part(want_w ? E : 0);
    float btotal = 0.f;
    for (int64_t r0 = 0; r0 < M; r0 += kRows) {
        const int64_t r1 = r0 + kRows < M ? r0 + kRows : M;
        if (want_w) part.assign(E, 0.f);
        float b = 0.f;
        for (int64_t r = r0; r < r1; ++r) {
            float d[27];
            for (int k = 0; k < 27; ++k) {
                const int32_t j = nbr[(int64_t)k * M + r];
                d[k] = (j >= 0 && (int64_t)j < M) ? ds[j] : 0.f;
            }
            const float g = dy ? sigmoid_f(s[r]) : 0.f;
            for (int c = 0; c < C; ++c) {
                float tsum = 0.f;
                for (int k = 0; k < 27; ++k) {
                    if (dx) tsum = tsum + d[k] * w[(26 - k) * C + c];
                    if (want_w) part[(26 - k) * C + c] = part[(26 - k) * C + c] + d[k] * x[r * C + c];
                }
                if (dx) dx[r * C + c] = dy ? dy[r * C + c] * g + tsum : tsum;
            }
            b = b + d[13];
        }
        if (want_w)
            for (int e = 0; e < E; ++e) total[e] = total[e] + part[e];
        btotal = btotal + b;
    }
    if (dw)
        for (int e = 0; e < E; ++e) dw[e] = total[e];
    if (dbias) dbias[0] = btotal;
    return SEG3D_OK;
}

}  // extern "C"
