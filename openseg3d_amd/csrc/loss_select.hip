// Cross-entropy with class weights and with hard-example selection (seg3d/models/losses/ohem_cross_entropy_loss.py:23-38,
// nn.CrossEntropyLoss(weight=...)) on float32 logits [n, c] with int64 labels: the options of the cross-entropy family
// that need more than a per-row pass.  Per valid row (label != ignore_index and in [0, c)) the loss is
//     l_r = w[y_r] * (lse_r - x_r[y_r]),   lse_r = m + log sum exp(x_r - m)                (w = 1 without class weights)
// in the expressions of criterion_device.hpp, by a thread that owns the row: nothing in l_r depends on where the row
// stands, so identical rows tie exactly.
//
//   MEAN_WEIGHTED  sum l / sum w[y]         MEAN_ALL  sum l / n_valid
//   THRESH         mean of l over the valid rows with softmax(x_r)[y_r] < keep_thresh (the unweighted probability)
//   RATIO          mean of the kept = (int64)((double)n_valid * keep_ratio) largest l (at most n_valid)
//
// RATIO is an exact top-k by radix select, without sorting and without a host read-back:
//   key_r    order-preserving uint32 of l_r: NaN above +inf (torch's sort order), -0 = +0, 0 on rows that are not valid
//            (the smallest key of a valid row is that of -inf, 0x007FFFFF);
//   pass 1   the cross-entropy pass: lse, key, and a histogram of the keys' top 11 bits;
//   pass 2-3 histograms of the next 11 and the last 10 bits over the rows that match the digits chosen so far;
//   pass 4   per-workgroup count of the rows whose key equals the threshold key T (the ties);
//   pass 5   a row is counted when key > T, or key == T and fewer than `admit` ties stand in front of it in row order
//            (the order of a stable descending sort); lse := +inf on the others, per-workgroup sums of the counted l;
//   finalize folds the workgroup sums in their order.
// Histograms are LDS counters flushed with integer atomics (they commute: the counts do not depend on arrival order).
// Every workgroup of pass k + 1 turns the histogram of pass k into the next digit and the number still to pick (a suffix
// scan over 2048 bins: cheaper than a one-workgroup launch in between); workgroup 0 records the result for later passes.
// Workgroups own contiguous row ranges, so the ties in front of a row are those of the workgroups in front plus those in
// front inside its own.  Sums: float64 per thread and from there on, fixed order, no floating-point atomics.
#include "criterion_device.hpp"

namespace {

using crit::kMaxBlocks;
using crit::kThreads;

constexpr int kBins = 2048;             // 11-bit digits (the last one has 10 bits and uses the lower half)
constexpr int kDigits = 3;
constexpr int kBinsPerThread = kBins / kThreads;
constexpr uint32_t kKeyNaN = 0xFFFFFFFFu;

__host__ __device__ constexpr int digit_shift(int d) { return d == 0 ? 21 : d == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bits(int d) { return d == 2 ? 10 : 11; }

struct SelectState {  // one per digit, written by workgroup 0 of the pass that follows the digit's histogram
    uint32_t prefix;  // the key's bits down to and including this digit
    uint32_t remain;  // rows still to pick among those that match prefix (after the last digit: ties to admit)
    uint32_t n_valid;
    uint32_t kept;
};

__device__ __forceinline__ uint32_t loss_key(float l) {
    if (l != l) return kKeyNaN;
    const uint32_t b = __float_as_uint(l == 0.f ? 0.f : l);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_loss(uint32_t k) {
    if (k == kKeyNaN) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// rows [row_begin, row_end) of this workgroup: the same split in every pass
__device__ __forceinline__ void block_rows(int64_t n, int64_t rows_per_block, int64_t* begin, int64_t* end) {
    const int64_t b = (int64_t)blockIdx.x * rows_per_block;
    const int64_t e = b + rows_per_block;
    *begin = b < n ? b : n;
    *end = e < n ? e : n;
}

__device__ __forceinline__ void hist_clear(uint32_t* lds_hist) {
    for (int i = threadIdx.x; i < kBins; i += kThreads) lds_hist[i] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void hist_flush(const uint32_t* lds_hist, uint32_t* __restrict__ hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += kThreads) {
        const uint32_t v = lds_hist[i];
        if (v) atomicAdd(&hist[i], v);
    }
}

// The step between two passes, by a whole workgroup: from the histogram of digit D over the rows that match the digits
// before it, and the number `remain` still to pick among them, the digit's value d with
//   count(digit > d) < remain <= count(digit >= d)
// and what is left to pick inside bin d.  For D = 0 the histogram holds every valid row: its total is n_valid, and
// remain = kept comes from it.  Nothing to pick (kept = 0): all-ones digits and remain 0, so that T = 0xFFFFFFFF with no
// tie admitted and no key above it.  Returns the state in every thread.
template <int D>
__device__ __forceinline__ SelectState select_digit(const uint32_t* __restrict__ hist, const SelectState* __restrict__ state,
                                                    double keep_ratio) {
    __shared__ SelectState result;
    uint32_t bins[kBinsPerThread];
    uint32_t own = 0;
    for (int j = 0; j < kBinsPerThread; ++j) {
        bins[j] = hist[threadIdx.x * kBinsPerThread + j];
        own += bins[j];
    }
    uint32_t total;
    const uint32_t inc = block_scan_inclusive<kThreads>(own, &total);
    const uint32_t above = total - inc;  // rows in the bins of the threads above this one
    SelectState prev;
    if constexpr (D == 0) {
        prev.prefix = 0u;
        prev.n_valid = total;
        // Python's int(n_valid * keep_ratio): the float64 product, truncated
        const double want = (double)total * keep_ratio;
        prev.kept = want >= (double)total ? total : (want > 0.0 ? (uint32_t)(int64_t)want : 0u);
        prev.remain = prev.kept;
    } else {
        prev = state[D - 1];
    }
    const uint32_t r = prev.remain;
    if (threadIdx.x == 0 && r == 0u) {
        result = prev;
        result.prefix = (prev.prefix << digit_bits(D)) | ((1u << digit_bits(D)) - 1u);
    }
    if (r > 0u && above < r && r <= above + own) {  // exactly one thread: r <= total by construction
        uint32_t acc = above;
        int d = 0;
        for (int j = kBinsPerThread - 1; j >= 0; --j) {
            if (acc + bins[j] >= r) {
                d = j;
                break;
            }
            acc += bins[j];
        }
        result = prev;
        result.prefix = (prev.prefix << digit_bits(D)) | (uint32_t)(threadIdx.x * kBinsPerThread + d);
        result.remain = r - acc;
    }
    __syncthreads();
    return result;
}

// ------------------------------------------------------------------------------------------------ the row pass
// MEAN_WEIGHTED, MEAN_ALL, THRESH: lse as the backward wants it and per-workgroup {sum l, denominator} at once.
// RATIO: lse of every row, the key, and the first histogram.
template <bool RATIO>
__global__ __launch_bounds__(kThreads) void row_pass_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                            int64_t n, int c, int64_t ignore_index,
                                                            const float* __restrict__ weight, int mode, float keep_thresh,
                                                            int64_t rows_per_block, float* __restrict__ lse,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                            double* __restrict__ part /*[gridDim.x][2]*/) {
    __shared__ uint32_t lds_hist[RATIO ? kBins : 1];
    if (RATIO) hist_clear(lds_hist);
    int64_t begin, end;
    block_rows(n, rows_per_block, &begin, &end);
    double loss = 0.0, den = 0.0;
    for (int64_t r = begin + threadIdx.x; r < end; r += kThreads) {
        const float* row = x + r * c;
        float m, s, l;
        crit::softmax_stats(row, c, &m, &s);
        const int64_t y = label[r];
        const bool counted = crit::ce_row(row, c, y, ignore_index, (!RATIO && mode == SEG3D_CE_SELECT_THRESH) ? keep_thresh : 0.f,
                                          m, s, &l);
        float w = 1.f, li = 0.f;
        if (counted) {
            if (weight) w = weight[y];
            li = w * (l - row[y]);
        }
        if (RATIO) {
            lse[r] = l;
            const uint32_t key = counted ? loss_key(li) : 0u;
            keys[r] = key;
            if (counted) atomicAdd(&lds_hist[key >> digit_shift(0)], 1u);
        } else {
            lse[r] = counted ? l : INFINITY;
            if (counted) {
                loss += (double)li;
                den += mode == SEG3D_CE_SELECT_MEAN_WEIGHTED ? (double)w : 1.0;
            }
        }
    }
    if (RATIO) {
        hist_flush(lds_hist, hist);
    } else {
        block_sum<kThreads>(loss, den);
        if (threadIdx.x == 0) {
            part[2 * blockIdx.x] = loss;
            part[2 * blockIdx.x + 1] = den;
        }
    }
}

// pass 2 (D = 1) and 3 (D = 2): digit D - 1 from its histogram, then the histogram of digit D over the matching rows
template <int D>
__global__ __launch_bounds__(kThreads) void digit_pass_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                              int64_t rows_per_block, double keep_ratio,
                                                              uint32_t* __restrict__ hists, SelectState* __restrict__ state) {
    __shared__ uint32_t lds_hist[kBins];
    const SelectState st = select_digit<D - 1>(hists + (D - 1) * kBins, state, keep_ratio);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[D - 1] = st;
    hist_clear(lds_hist);
    int64_t begin, end;
    block_rows(n, rows_per_block, &begin, &end);
    for (int64_t r = begin + threadIdx.x; r < end; r += kThreads) {
        const uint32_t key = keys[r];
        if (key != 0u && (key >> digit_shift(D - 1)) == st.prefix)
            atomicAdd(&lds_hist[(key >> digit_shift(D)) & ((1u << digit_bits(D)) - 1u)], 1u);
    }
    hist_flush(lds_hist, hists + D * kBins);
}

// pass 4: the last digit gives the threshold key T = prefix and the ties to admit; this workgroup's rows with key == T
__global__ __launch_bounds__(kThreads) void tie_count_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                             int64_t rows_per_block, const uint32_t* __restrict__ hists,
                                                             SelectState* __restrict__ state,
                                                             uint32_t* __restrict__ tie_count /*[gridDim.x]*/) {
    const SelectState st = select_digit<kDigits - 1>(hists + (kDigits - 1) * kBins, state, 0.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[kDigits - 1] = st;
    int64_t begin, end;
    block_rows(n, rows_per_block, &begin, &end);
    uint32_t mine = 0;
    for (int64_t r = begin + threadIdx.x; r < end; r += kThreads) mine += keys[r] == st.prefix ? 1u : 0u;
    uint32_t total;
    block_scan_inclusive<kThreads>(mine, &total);
    if (threadIdx.x == 0) tie_count[blockIdx.x] = total;
}

// pass 5: who is counted
__global__ __launch_bounds__(kThreads) void select_rows_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                               int64_t rows_per_block, const SelectState* __restrict__ state,
                                                               const uint32_t* __restrict__ tie_count,
                                                               float* __restrict__ lse, double* __restrict__ part) {
    const uint32_t T = state[kDigits - 1].prefix, admit = state[kDigits - 1].remain;
    uint32_t before = 0;  // ties in the workgroups in front of this one
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kThreads) before += tie_count[b];
    uint32_t ties_before;
    block_scan_inclusive<kThreads>(before, &ties_before);
    int64_t begin, end;
    block_rows(n, rows_per_block, &begin, &end);
    double loss = 0.0;
    for (int64_t r0 = begin; r0 < end; r0 += kThreads) {  // every thread walks every chunk: the scan has barriers
        const int64_t r = r0 + threadIdx.x;
        const uint32_t key = r < end ? keys[r] : 0u;
        const bool tie = key != 0u && key == T;
        uint32_t chunk_ties;
        const uint32_t inc = block_scan_inclusive<kThreads>(tie ? 1u : 0u, &chunk_ties);
        const bool counted = key != 0u && (key > T || (tie && ties_before + inc - 1u < admit));
        if (r < end) {
            if (counted)
                loss += (double)key_loss(key);
            else
                lse[r] = INFINITY;
        }
        ties_before += chunk_ties;
    }
    const double a = block_sum<kThreads>(loss);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = a;
        part[2 * blockIdx.x + 1] = 0.0;
    }
}

// stats = {sum l / denominator (0 when the denominator is 0), denominator}; RATIO takes kept for the denominator
__global__ __launch_bounds__(kThreads) void select_finalize_kernel(const double* __restrict__ part, int nblocks,
                                                                   const SelectState* __restrict__ state,
                                                                   float* __restrict__ stats) {
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, SEG3D_WAVE);
        b += __shfl_xor(b, off, SEG3D_WAVE);
    }
    __shared__ double red[2][kThreads / 64];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0;
        b = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) {
            a += red[0][w];
            b += red[1][w];
        }
        if (state) b = (double)state[kDigits - 1].kept;
        stats[0] = b != 0.0 ? (float)(a / b) : 0.f;
        stats[1] = (float)b;
    }
}

__global__ __launch_bounds__(kThreads) void select_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                              const float* __restrict__ weight,
                                                              const float* __restrict__ lse, const float* __restrict__ stats,
                                                              const float* __restrict__ gout, int64_t n, int c,
                                                              float* __restrict__ dx) {
    const float den = stats[1];
    const float scale = den != 0.f ? gout[0] / den : 0.f;
    const int64_t total = n * c;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t r = e / c;
        const int j = (int)(e - r * c);
        const float l = lse[r];
        float g = 0.f;
        if (l != INFINITY && scale != 0.f) {  // a counted row: its label is in [0, c)
            const int64_t y = label[r];
            g = crit::ce_grad(x[e], l, j == y, weight ? weight[y] * scale : scale);
        }
        dx[e] = g;
    }
}

struct Plan {
    int nb;
    int64_t rows_per_block;
};

static inline Plan make_plan(int64_t n) {
    Plan p;
    int64_t nb = ceil_div64(n, kThreads);
    if (nb > kMaxBlocks) nb = kMaxBlocks;
    p.nb = (int)nb;
    p.rows_per_block = nb > 0 ? ceil_div64(ceil_div64(n, nb), kThreads) * kThreads : kThreads;
    return p;
}

static inline bool mode_ok(int32_t mode) { return mode >= SEG3D_CE_SELECT_MEAN_WEIGHTED && mode <= SEG3D_CE_SELECT_RATIO; }

constexpr int64_t kMaxRows = 0x7FFFFFFF;  // the counters are uint32

}  // namespace

// partials [kMaxBlocks][2] double | histograms [3][2048] u32 | state [3] | tie counts [kMaxBlocks] u32 | keys [n] u32
extern "C" size_t seg3d_ce_select_workspace_bytes(int64_t n) {
    if (n < 0 || n > kMaxRows) return 0;
    return align_up((size_t)kMaxBlocks * 2 * sizeof(double), 256) + align_up((size_t)kDigits * kBins * sizeof(uint32_t), 256) +
           align_up((size_t)kDigits * sizeof(SelectState), 256) + align_up((size_t)kMaxBlocks * sizeof(uint32_t), 256) +
           align_up((size_t)(n > 0 ? n : 1) * sizeof(uint32_t), 256);
}

extern "C" int seg3d_ce_select_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index,
                                   const float* class_weight, int32_t mode, float keep_thresh, double keep_ratio, float* lse,
                                   float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || n > kMaxRows || c <= 0 || c > 4096 || !mode_ok(mode) || !stats || !workspace ||
        workspace_bytes < seg3d_ce_select_workspace_bytes(n))
        return SEG3D_EINVAL;
    if (mode == SEG3D_CE_SELECT_THRESH && !(keep_thresh > 0.f)) return SEG3D_EINVAL;
    if (mode == SEG3D_CE_SELECT_RATIO && !(keep_ratio > 0.0)) return SEG3D_EINVAL;
    if (n > 0 && (!logits || !labels || !lse)) return SEG3D_EINVAL;
    hipStream_t st = as_stream(stream);
    WsCarver ws(workspace);
    double* part = ws.take<double>((size_t)kMaxBlocks * 2);
    uint32_t* hists = ws.take<uint32_t>((size_t)kDigits * kBins);
    SelectState* state = ws.take<SelectState>(kDigits);
    uint32_t* tie_count = ws.take<uint32_t>(kMaxBlocks);
    uint32_t* keys = ws.take<uint32_t>((size_t)(n > 0 ? n : 1));
    const Plan p = make_plan(n);
    const dim3 grid((unsigned)p.nb), block(kThreads);
    if (mode != SEG3D_CE_SELECT_RATIO || p.nb == 0) {
        if (p.nb > 0) {
            hipLaunchKernelGGL(row_pass_kernel<false>, grid, block, 0, st, logits, labels, n, c, ignore_index, class_weight,
                               mode, keep_thresh, p.rows_per_block, lse, keys, hists, part);
            SEG3D_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(select_finalize_kernel, dim3(1), block, 0, st, part, p.nb, (const SelectState*)nullptr, stats);
        SEG3D_CHECK_LAUNCH();
        return SEG3D_OK;
    }
    SEG3D_CHECK_HIP(hipMemsetAsync(hists, 0, (size_t)kDigits * kBins * sizeof(uint32_t), st));
    hipLaunchKernelGGL(row_pass_kernel<true>, grid, block, 0, st, logits, labels, n, c, ignore_index, class_weight, mode,
                       keep_thresh, p.rows_per_block, lse, keys, hists, part);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(digit_pass_kernel<1>, grid, block, 0, st, keys, n, p.rows_per_block, keep_ratio, hists, state);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(digit_pass_kernel<2>, grid, block, 0, st, keys, n, p.rows_per_block, keep_ratio, hists, state);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(tie_count_kernel, grid, block, 0, st, keys, n, p.rows_per_block, hists, state, tie_count);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_rows_kernel, grid, block, 0, st, keys, n, p.rows_per_block, state, tie_count, lse, part);
    SEG3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_finalize_kernel, dim3(1), block, 0, st, part, p.nb, (const SelectState*)state, stats);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_ce_select_bwd(const float* logits, const int64_t* labels, const float* class_weight, const float* lse,
                                   const float* stats, const float* grad_out, int64_t n, int32_t c, int32_t mode,
                                   float* dlogits, void* stream) {
    if (n < 0 || n > kMaxRows || c <= 0 || c > 4096 || !mode_ok(mode) || !stats || !grad_out) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    if (!logits || !labels || !lse || !dlogits) return SEG3D_EINVAL;
    int64_t nb = ceil_div64(n * c, (int64_t)kThreads * 4);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(select_bwd_kernel, dim3((unsigned)nb), dim3(kThreads), 0, as_stream(stream), logits, labels,
                       class_weight, lse, stats, grad_out, n, c, dlogits);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}
