// Dense Linear weight gradient, LDS-shared form (round 5; VERDICT r4 item 2 ii: "output blocks with the x slab shared by
// the waves"):   dw[co][ci] = sum_r dy[r][co] * x[r][ci],   db[co] = sum_r dy[r][co]
//
// wgrad_dense.hip feeds every 64 x 64 block straight from global memory: a C x C gradient re-reads each row C / 64 times
// per operand, and that L2 -> L1 stream (~10 TB/s) is what bounds it (192 x 192 @58 k rows: 269 MB through the L1s for
// 90 MB of operands).  Here a workgroup of WA x WB waves owns a (96 WA) x (48 WB) block -- wave tile 96 (co) x 48 (ci),
// 18 accumulator tiles -- over one chunk of rows.  Per 32-row step all threads fetch the block's dy and x slabs ONCE
// (16-byte pieces, whole 64-byte sectors per instruction), split them into bf16 hi | lo and park four row-major planes in
// LDS; the waves read their K-major MFMA fragments back with ds_read_b64_tr_b16 (the hardware transpose the attention
// kernels use: nothing is stored transposed).  192 x 192: 2 blocks x (192 + 96) columns per row = 576 column reads per row
// instead of 1 152.  One image buffer, two barriers per step (the next step's rows are already in flight in registers);
// two to three workgroups per CU cover each other's barriers.
//
// The price is the partial sums: every workgroup holds a whole block and writes it once per chunk, so the partial blocks
// are (workgroups x block) instead of a quarter of that (wgrad_dense.hip sums its four waves through LDS first).  The
// plan keeps one resident round of workgroups; wgrad_chunk_reduce / reduce_partials_batched sum the chunks in a fixed order
// as before: no atomics, bit-reproducible run to run.  db rides in the matrix pipe: a fragment of ones against the dy
// fragments (hi and lo: the column sum of the split operand, 2^-17 relative per element), in the waves of the first ci block.
#include <atomic>
#include <type_traits>

#include "split_bf16.hpp"

namespace {

using namespace sbf;

// row stride in bytes of a plane with `c` bf16 columns: an odd multiple of 32 bytes, so that the 16 rows a transposed read
// touches (32 contiguous bytes each) fall into 16 different bank groups
constexpr int row_stride(int c) { return c * 2 + (((c * 2 / 32) & 1) ? 0 : 32); }

template <int WA, int WB>
__global__ __launch_bounds__(64 * WA * WB, 2) void wgrad_dense_lds_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                          int64_t m_rows, int cin, int cout, int rows_per_chunk,
                                                                          int nbi, int n_blocks, float* __restrict__ part,
                                                                          int want_bias) {
    constexpr int NT = 64 * WA * WB;
    constexpr int DYC = 96 * WA, XC = 48 * WB;  // the block's columns of dy (co) and x (ci)
    constexpr int RSY = row_stride(DYC), RSX = row_stride(XC);
    constexpr int PY = 32 * RSY, PX = 32 * RSX;  // one plane
    constexpr int Q = (DYC + XC) / 4;            // 16-byte pieces per row of the step's slabs
    constexpr int NP = 32 * Q / NT;              // pieces per thread and step
    static_assert(32 * Q % NT == 0, "pieces divide among the threads");
    __shared__ __attribute__((aligned(16))) char lds[2 * PY + 2 * PX];  // dy hi | dy lo | x hi | x lo
    char* const y_hi = lds;
    char* const x_hi = lds + 2 * PY;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c16 = lane & 15;
    const int wa = wave / WB, wb = wave % WB;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int chunk = (k / n_blocks) * 8 + xcd, blk = k % n_blocks;
    const int bi = blk % nbi, bo = blk / nbi;
    const int co0 = bo * DYC, ci0 = bi * XC;
    const int64_t r_begin = (int64_t)chunk * rows_per_chunk;
    if (r_begin >= m_rows) return;  // padding of the XCD-aligned grid (whole workgroup)
    const int64_t r_end = r_begin + rows_per_chunk < m_rows ? r_begin + rows_per_chunk : m_rows;
    const int n_steps = (int)((r_end - r_begin + 31) / 32);
    const bool want_db = want_bias && bi == 0 && wb == 0;  // (wave-uniform)

    f32x4 acc[3][6];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 dbacc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) dbacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // piece i of this thread: p = tid + NT * i -> (row = p / Q, q = p % Q): q < DYC / 4 is a dy piece, the rest x pieces
    f32x4 raw[NP];
    auto load_step = [&](int s) {
        const int64_t r0 = r_begin + 32 * (int64_t)s;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = tid + NT * i;
            const int row = p / Q, q = p - row * Q;
            const bool is_y = q < DYC / 4;
            int64_t r = r0 + row;
            const bool ok = r < r_end;
            r = ok ? r : r_end - 1;
            const float* src = is_y ? dy + r * cout + co0 + 4 * q : x + r * cin + ci0 + 4 * (q - DYC / 4);
            const f32x4 v = *reinterpret_cast<const f32x4*>(src);
            raw[i] = ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = tid + NT * i;
            const int row = p / Q, q = p - row * Q;
            const bool is_y = q < DYC / 4;
            char* dst = is_y ? y_hi + row * RSY + q * 8 : x_hi + row * RSX + (q - DYC / 4) * 8;
            const int plane = is_y ? PY : PX;
            uint32_t h0, l0, h1, l1;
            split2(raw[i][0], raw[i][1], &h0, &l0);
            split2(raw[i][2], raw[i][3], &h1, &l1);
            *reinterpret_cast<u32x2*>(dst) = (u32x2){h0, h1};
            *reinterpret_cast<u32x2*>(dst + plane) = (u32x2){l0, l1};
        }
    };
    // K-major fragment of 16 columns starting at col0 of a row-major plane: lane (c16, g) ends up with column col0 + c16,
    // rows {4 g .. 4 g + 3, 16 + 4 g .. 16 + 4 g + 3} (the same row order for both operands)
    auto read_tr = [&](const char* plane, int rs, int col0) {
        const int qq = c16 >> 2, pp = c16 & 3;
        const char* p0 = plane + (4 * g + qq) * rs + (col0 + 4 * pp) * 2;
        const s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0));
        const s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + 16 * rs));
        return __builtin_bit_cast(bf16x8, (s16x8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]});
    };
    const u32x4 ones_w = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_w);

    load_step(0);
    for (int s = 0; s < n_steps; ++s) {
        store_step();
        __syncthreads();  // the step's image is complete
        if (s + 1 < n_steps) load_step(s + 1);  // in flight under the MFMAs below
        bf16x8 xh[3], xl[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            xh[j] = read_tr(x_hi, RSX, 48 * wb + 16 * j);
            xl[j] = read_tr(x_hi + PX, RSX, 48 * wb + 16 * j);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const bf16x8 yh = read_tr(y_hi, RSY, 96 * wa + 16 * i);
            const bf16x8 yl = read_tr(y_hi + PY, RSY, 96 * wa + 16 * i);
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j][i] = mfma3(xh[j], xl[j], yh, yl, acc[j][i]);
            if (want_db) {
                dbacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, yl, dbacc[i], 0, 0, 0);
                dbacc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, yh, dbacc[i], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave is done with the image
    }

    // partial of this chunk: [cout][cin] block sums followed by [cout] column sums of dy.
    // acc[j][i] of lane (c16, g) = dw[co0 + 96 wa + 16 i + c16][ci0 + 48 wb + 16 j + 4 g .. + 3]
    float* pw = part + (int64_t)chunk * ((int64_t)cout * cin + cout);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int co = co0 + 96 * wa + 16 * i + c16;
#pragma unroll
        for (int j = 0; j < 3; ++j) *reinterpret_cast<f32x4*>(pw + (int64_t)co * cin + ci0 + 48 * wb + 16 * j + 4 * g) = acc[j][i];
        if (want_db && g == 0) pw[(int64_t)cout * cin + co] = dbacc[i][0];
    }
}

// SEG3D_WGRAD_LDS=1 (A/B, OFF by default: it did not win); SEG3D_WGRAD_LDS_TARGET: workgroups the plan aims at (default 512).
// Measured (tools/wgrad_bench.py, one box, wgrad_dense.hip -> this kernel; partial blocks alone | with their fixed-order sum):
// 192 -> 192 @58 k rows 31.0 -> 34.3 | 29.9 -> 43.5 us, 192 -> 384 55.5 -> 53.6 | 53.1 -> 62.6, 384 -> 192 50.3 -> 55.5 |
// 51.9 -> 60.7, 96 -> 192 @121 k 33.0 -> 31.6 | 37.4 -> 45.1, 384 -> 768 @19 k 71.7 -> 66.7 | 72.1 -> 71.8, 384 -> 384 37.4 ->
// 36.6 | 40.4 -> 43.3; the family 3.70 -> 3.70 ms alone, 3.90 -> 4.41 ms with the sums (256 or 1 024 workgroups: 4.9 ms).
// Half the L2 -> L1 row traffic and a third of the split instructions bought nothing: the direct-to-fragment kernel is not
// bound by either (DESIGN.md section 6 had said the stream was the bound), and the four times larger partial blocks (34 - 36 MB
// per launch against 8 - 17) cost what the reduce then pays.  Kept as a parity-tested experiment.
static const int g_lds_on = env_int("SEG3D_WGRAD_LDS", 0) == 1 ? 1 : 0;
static const int g_lds_target = env_int_in("SEG3D_WGRAD_LDS_TARGET", 64, 4096, 512);

// seg3d_debug_set_wgrad_lds (parity tests pin the opt-in kernel with it): 1 = on, 0 = off, -1 = the environment's choice
static std::atomic<int> g_lds_forced{-1};

}  // namespace

extern "C" int seg3d_debug_set_wgrad_lds(int32_t on) {
    if (on < -1 || on > 1) return SEG3D_EINVAL;
    g_lds_forced.store(on, std::memory_order_relaxed);
    return SEG3D_OK;
}

// 1 when the LDS-shared kernel takes this shape (then *chunks / *rows describe its partial blocks), 0 otherwise
int wgrad_dense_lds_plan(int64_t m, int cin, int cout, int* chunks, int64_t* rows) {
    // (the 1 x 2 / 2 x 1 / 1 x 1 wave arrangements for cout % 192 or cin % 96 != 0 hold 12 - 18 pieces per thread and spill:
    // those shapes stay on wgrad_dense.hip)
    const int forced = g_lds_forced.load(std::memory_order_relaxed);
    if (!(forced < 0 ? g_lds_on : forced) || m < 4096 || cout % 192 || cin % 96) return 0;
    const int wa = 2, wb = 2;
    const int n_blocks = (cout / (96 * wa)) * (cin / (48 * wb));
    int64_t c = g_lds_target / n_blocks / 8 * 8;
    if (c < 8) c = 8;
    int64_t r = (m + c - 1) / c;
    if (r < 128) r = 128;
    r = (r + 31) / 32 * 32;
    *rows = r;
    *chunks = (int)((m + r - 1) / r);
    return 1;
}

int wgrad_dense_lds_launch(const float* x, const float* dy, int64_t m, int cin, int cout, int chunks, int64_t rows, float* part,
                           int want_bias, hipStream_t st) {
    const int nbi = cin / 96, n_blocks = (cout / 192) * nbi;
    const unsigned blocks = (unsigned)((chunks + 7) / 8 * 8) * (unsigned)n_blocks;
    hipLaunchKernelGGL((wgrad_dense_lds_kernel<2, 2>), dim3(blocks), dim3(256), 0, st, x, dy, m, cin, cout, (int)rows, nbi, n_blocks,
                       part, want_bias);
    return 0;
}
