// FocalLoss and DiceLoss of the reference (seg3d/models/losses/focal_loss.py:51-92, dice_loss.py:9-43, 84-114,
// seg3d/utils/loss_utils.py:43-73) on float32 logits [n, C <= 64] with int64 labels, forward and backward.  Composed
// from torch ops either loss costs about ten [n, C] temporaries per direction; here each direction is one pass over the
// logits and nothing [n, C] is kept between them.  Reductions: per-thread float32 sums, float64 from the wave shuffle
// on, per-workgroup partials, and a finalize kernel that adds the partials in a fixed order -- no floating-point
// atomics, two runs give the same bits.
//
// Focal (elementwise, a thread strides over the n * C elements, coalesced).  Rows with label == ignore_index or outside
// [0, C) take no part (the reference's one_hot raises on the latter).  With t = [j == y], z = t ? -x : x:
//     bce = softplus(z) = max(z, 0) + log1p(exp(-|z|)),    q = 1 - p_t = sigmoid(z)       (no 1 - sigmoid cancellation)
//     loss = alpha_t * w_j * bce * q^gamma,                alpha_t = t ? alpha : 1 - alpha  (1 when alpha < 0)
//     d loss / dz = alpha_t * w_j * q^gamma * (q + gamma * bce * (1 - q)),   dx = -dz for t = 1
//   mean = sum / (n_valid * C), 0 when no row is valid.
//
// Dice (a thread owns a row; a workgroup moves its 128 rows through LDS so that global reads and writes are coalesced,
// LDS row stride C | 1 keeps the row walks off a common bank).  With p = softmax(x_r), t = onehot(clamp(y_r, 0, C-1)),
// v_r = [y_r != ignore_index], S = loss_weight / (C * n) (/ (avg_factor + eps) when avg_factor is given):
//     L = S * sum_r sum_{i != ignore_index} w_i * (1 - (2 p t v + smooth) / (p^e + t^e + smooth))
//     g_i = dL/dp_i = S * w_i * (num * e * p^(e-1) / den^2 - 2 t v / den),   dx_j = p_j * (g_j - sum_i g_i p_i)
//   The mean runs over all n rows and v masks the numerator only: ignored rows have a gradient (dice_loss.py:40-41).
#include <float.h>
#include <math.h>

#include "wave_ops.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kDiceRows = 128;  // rows (= threads) of a dice workgroup: 128 * 65 floats of LDS at C = 64

// ---------------------------------------------------------------------------------------------------- focal
enum { kGammaZero = 0, kGammaOne = 1, kGammaTwo = 2, kGammaAny = 3 };

static inline int gamma_mode(float gamma) {
    return gamma == 0.f ? kGammaZero : gamma == 1.f ? kGammaOne : gamma == 2.f ? kGammaTwo : kGammaAny;
}

__device__ __forceinline__ float pow_gamma(float q, float gamma, int gmode) {
    switch (gmode) {
        case kGammaZero: return 1.f;
        case kGammaOne: return q;
        case kGammaTwo: return q * q;
        default: return powf(q, gamma);
    }
}

struct FocalTerm {
    float bce, q, one_minus_q, coef;  // coef = alpha_t * w_j
};

__device__ __forceinline__ FocalTerm focal_term(float x, bool t, float alpha, float w) {
    const float z = t ? -x : x;
    const float em = expf(-fabsf(z));
    const float inv = 1.f / (1.f + em);
    FocalTerm f;
    f.bce = fmaxf(z, 0.f) + log1pf(em);
    f.q = z >= 0.f ? inv : em * inv;
    f.one_minus_q = z >= 0.f ? em * inv : inv;
    f.coef = alpha >= 0.f ? (t ? alpha : 1.f - alpha) * w : w;
    return f;
}

__device__ __forceinline__ int64_t row_of(int64_t e, int c, bool small) {
    return small ? (int64_t)((uint32_t)e / (uint32_t)c) : e / c;
}

__global__ __launch_bounds__(kThreads) void focal_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                             int64_t n, int c, int64_t ignore_index, float gamma, int gmode,
                                                             float alpha, const float* __restrict__ weight,
                                                             double* __restrict__ part /*[gridDim.x][2]*/) {
    const int64_t total = n * c;
    const bool small = total < ((int64_t)1 << 32);
    float loss = 0.f, cnt = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t r = row_of(e, c, small);
        const int j = (int)(e - r * c);
        const int64_t y = label[r];
        if (y == ignore_index || y < 0 || y >= c) continue;
        const FocalTerm f = focal_term(x[e], j == y, alpha, weight ? weight[j] : 1.f);
        loss += f.coef * f.bce * pow_gamma(f.q, gamma, gmode);
        if (j == 0) cnt += 1.f;
    }
    double a = loss, b = cnt;
    block_sum<kThreads>(a, b);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = a;
        part[2 * blockIdx.x + 1] = b;
    }
}

// stats[0] = sum, or sum / (n_valid * c) for the mean (0 when no row is valid); stats[1] = n_valid
__global__ __launch_bounds__(kThreads) void focal_finalize_kernel(const double* __restrict__ part, int nblocks, int c,
                                                                  int mean, float* __restrict__ stats) {
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    block_sum<kThreads>(a, b);
    if (threadIdx.x == 0) {
        stats[0] = (float)(mean ? (b > 0.0 ? a / (b * c) : 0.0) : a);
        stats[1] = (float)b;
    }
}

__global__ __launch_bounds__(kThreads) void focal_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                             const float* __restrict__ stats, const float* __restrict__ gout,
                                                             int64_t n, int c, int64_t ignore_index, float gamma, int gmode,
                                                             float alpha, const float* __restrict__ weight, int mean,
                                                             float* __restrict__ dx) {
    const float cnt = stats[1];
    const float scale = mean ? (cnt > 0.f ? gout[0] / (cnt * (float)c) : 0.f) : gout[0];
    const int64_t total = n * c;
    const bool small = total < ((int64_t)1 << 32);
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t r = row_of(e, c, small);
        const int j = (int)(e - r * c);
        const int64_t y = label[r];
        float g = 0.f;
        if (y != ignore_index && y >= 0 && y < c) {
            const bool t = j == y;
            const FocalTerm f = focal_term(x[e], t, alpha, weight ? weight[j] : 1.f);
            const float dz = f.coef * pow_gamma(f.q, gamma, gmode) * (f.q + gamma * f.bce * f.one_minus_q);
            g = (t ? -dz : dz) * scale;
        }
        dx[e] = g;
    }
}

// ---------------------------------------------------------------------------------------------------- dice
enum { kExpOne = 1, kExpTwo = 2, kExpAny = 3 };

static inline int exponent_mode(float e) { return e == 1.f ? kExpOne : e == 2.f ? kExpTwo : kExpAny; }

struct DiceArgs {
    int c;
    int64_t ignore_index;
    float smooth, exponent;
    int emode;
    float t0e;  // 0^exponent, the one-hot's off entries raised like the reference raises them
};

// walks the rows * c contiguous floats of a tile: f(i, k) with i the offset in global memory and k = r * cs + j the
// one in the LDS tile (row stride cs); (r, j) follow i without a division per element
template <class F>
__device__ __forceinline__ void dice_walk_tile(int rows, int c, int cs, F f) {
    const int count = rows * c;
    const int dq = kDiceRows / c, dr = kDiceRows % c;
    int r = (int)threadIdx.x / c, j = (int)threadIdx.x % c;
    for (int i = threadIdx.x; i < count; i += kDiceRows) {
        f(i, r * cs + j);
        r += dq;
        j += dr;
        if (j >= c) {
            j -= c;
            ++r;
        }
    }
}

// row <- exp(row - max); returns 1 / sum
__device__ __forceinline__ float dice_row_exp(float* row, int c) {
    float m = row[0];
    for (int j = 1; j < c; ++j) m = fmaxf(m, row[j]);
    float s = 0.f;
    for (int j = 0; j < c; ++j) {
        const float e = expf(row[j] - m);
        row[j] = e;
        s += e;
    }
    return 1.f / s;
}

__device__ __forceinline__ void dice_num_den(float p, bool t, float v, const DiceArgs& a, float& num, float& den) {
    const float pe = a.emode == kExpOne ? p : a.emode == kExpTwo ? p * p : powf(p, a.exponent);
    num = (t ? 2.f * p * v : 0.f) + a.smooth;
    den = pe + (t ? 1.f : a.t0e) + a.smooth;
}

__global__ __launch_bounds__(kDiceRows) void dice_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                             int64_t n, DiceArgs a, const float* __restrict__ weight,
                                                             double* __restrict__ part /*[gridDim.x]*/) {
    extern __shared__ float tile[];
    const int c = a.c, cs = c | 1;
    float acc = 0.f;
    for (int64_t row0 = (int64_t)blockIdx.x * kDiceRows; row0 < n; row0 += (int64_t)gridDim.x * kDiceRows) {
        const int rows = (int)(n - row0 < kDiceRows ? n - row0 : kDiceRows);
        const float* src = x + row0 * c;
        dice_walk_tile(rows, c, cs, [&](int i, int k) { tile[k] = src[i]; });
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* row = tile + threadIdx.x * cs;
            const int64_t y = label[row0 + threadIdx.x];
            const int yc = (int)(y < 0 ? 0 : y > c - 1 ? c - 1 : y);
            const float v = y != a.ignore_index ? 1.f : 0.f;
            const float inv = dice_row_exp(row, c);
            for (int j = 0; j < c; ++j) {
                if (j == a.ignore_index) continue;
                float num, den;
                dice_num_den(row[j] * inv, j == yc, v, a, num, den);
                acc += (weight ? weight[j] : 1.f) * (1.f - num / den);
            }
        }
        __syncthreads();
    }
    double s = acc, unused = 0.0;
    block_sum<kDiceRows>(s, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void dice_finalize_kernel(const double* __restrict__ part, int nblocks, double scale,
                                                                 float* __restrict__ out) {
    double a = 0.0, unused = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) a += part[i];
    block_sum<kThreads>(a, unused);
    if (threadIdx.x == 0) out[0] = (float)(a * scale);
}

__global__ __launch_bounds__(kDiceRows) void dice_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                             const float* __restrict__ gout, int64_t n, DiceArgs a,
                                                             const float* __restrict__ weight, float scale,
                                                             float* __restrict__ dx) {
    extern __shared__ float tile[];
    const int c = a.c, cs = c | 1;
    const float up = gout[0] * scale;
    for (int64_t row0 = (int64_t)blockIdx.x * kDiceRows; row0 < n; row0 += (int64_t)gridDim.x * kDiceRows) {
        const int rows = (int)(n - row0 < kDiceRows ? n - row0 : kDiceRows);
        const float* src = x + row0 * c;
        dice_walk_tile(rows, c, cs, [&](int i, int k) { tile[k] = src[i]; });
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* row = tile + threadIdx.x * cs;
            const int64_t y = label[row0 + threadIdx.x];
            const int yc = (int)(y < 0 ? 0 : y > c - 1 ? c - 1 : y);
            const float v = y != a.ignore_index ? 1.f : 0.f;
            const float inv = dice_row_exp(row, c);
            // g_j = dL/dp_j (without the upstream factor); the second walk recomputes it instead of keeping a second row
            auto grad_p = [&](int j, float p) {
                if (j == a.ignore_index) return 0.f;
                const bool t = j == yc;
                float num, den;
                dice_num_den(p, t, v, a, num, den);
                const float dpe = a.emode == kExpOne ? 1.f : a.emode == kExpTwo ? 2.f * p : a.exponent * powf(p, a.exponent - 1.f);
                return (weight ? weight[j] : 1.f) * (num * dpe / (den * den) - (t ? 2.f * v : 0.f) / den);
            };
            float dot = 0.f;
            for (int j = 0; j < c; ++j) {
                const float p = row[j] * inv;
                row[j] = p;
                dot += grad_p(j, p) * p;
            }
            for (int j = 0; j < c; ++j) {
                const float p = row[j];
                row[j] = up * p * (grad_p(j, p) - dot);
            }
        }
        __syncthreads();
        float* dst = dx + row0 * c;
        dice_walk_tile(rows, c, cs, [&](int i, int k) { dst[i] = tile[k]; });
        __syncthreads();
    }
}

static inline bool dice_args(int32_t c, int64_t ignore_index, float smooth, float exponent, DiceArgs* a) {
    if (c <= 0 || c > 64 || !(smooth == smooth) || !(exponent == exponent)) return false;
    a->c = c;
    a->ignore_index = ignore_index;
    a->smooth = smooth;
    a->exponent = exponent;
    a->emode = exponent_mode(exponent);
    a->t0e = powf(0.f, exponent);
    return true;
}

// loss_weight / (c * n), over (avg_factor + eps) when avg_factor >= 0 (loss_utils.py:65-69); 0 for an empty input
static inline double dice_scale(int64_t n, int32_t c, float loss_weight, float avg_factor) {
    if (n == 0) return 0.0;
    double s = (double)loss_weight / ((double)c * (double)n);
    if (avg_factor >= 0.f) s /= (double)avg_factor + (double)FLT_EPSILON;
    return s;
}

static inline int dice_blocks(int64_t n) {
    const int64_t nb = ceil_div64(n, kDiceRows);
    return (int)(nb > kMaxBlocks ? kMaxBlocks : nb);
}

}  // namespace

extern "C" size_t seg3d_pointwise_loss_workspace_bytes(int64_t n) {
    return n < 0 ? 0 : (size_t)kMaxBlocks * 2 * sizeof(double);
}

extern "C" int seg3d_focal_loss_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index,
                                    float gamma, float alpha, const float* class_weight, int32_t reduction, float* stats,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || c <= 0 || c > 64 || !(gamma >= 0.f) || !stats || !workspace ||
        (reduction != SEG3D_REDUCE_SUM && reduction != SEG3D_REDUCE_MEAN) ||
        workspace_bytes < seg3d_pointwise_loss_workspace_bytes(n))
        return SEG3D_EINVAL;
    if (n > 0 && (!logits || !labels)) return SEG3D_EINVAL;
    hipStream_t st = as_stream(stream);
    double* part = static_cast<double*>(workspace);
    int64_t nb = ceil_div64(n * c, kThreads);
    if (nb > kMaxBlocks) nb = kMaxBlocks;
    if (nb > 0) {
        hipLaunchKernelGGL(focal_fwd_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, logits, labels, n, c, ignore_index,
                           gamma, gamma_mode(gamma), alpha, class_weight, part);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(kThreads), 0, st, part, (int)nb, c,
                       reduction == SEG3D_REDUCE_MEAN ? 1 : 0, stats);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_focal_loss_bwd(const float* logits, const int64_t* labels, const float* stats, const float* grad_out,
                                    int64_t n, int32_t c, int64_t ignore_index, float gamma, float alpha,
                                    const float* class_weight, int32_t reduction, float* dlogits, void* stream) {
    if (n < 0 || c <= 0 || c > 64 || !(gamma >= 0.f) || !stats || !grad_out ||
        (reduction != SEG3D_REDUCE_SUM && reduction != SEG3D_REDUCE_MEAN))
        return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    if (!logits || !labels || !dlogits) return SEG3D_EINVAL;
    int64_t nb = ceil_div64(n * c, (int64_t)kThreads * 4);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(focal_bwd_kernel, dim3((unsigned)nb), dim3(kThreads), 0, as_stream(stream), logits, labels, stats,
                       grad_out, n, c, ignore_index, gamma, gamma_mode(gamma), alpha, class_weight,
                       reduction == SEG3D_REDUCE_MEAN ? 1 : 0, dlogits);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_dice_loss_fwd(const float* logits, const int64_t* labels, int64_t n, int32_t c, int64_t ignore_index,
                                   float smooth, float exponent, const float* class_weight, float loss_weight,
                                   float avg_factor, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
    DiceArgs a;
    if (n < 0 || !dice_args(c, ignore_index, smooth, exponent, &a) || !loss || !workspace ||
        workspace_bytes < seg3d_pointwise_loss_workspace_bytes(n))
        return SEG3D_EINVAL;
    if (n > 0 && (!logits || !labels)) return SEG3D_EINVAL;
    hipStream_t st = as_stream(stream);
    double* part = static_cast<double*>(workspace);
    const int nb = dice_blocks(n);
    if (nb > 0) {
        hipLaunchKernelGGL(dice_fwd_kernel, dim3((unsigned)nb), dim3(kDiceRows), (size_t)kDiceRows * (c | 1) * sizeof(float),
                           st, logits, labels, n, a, class_weight, part);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(kThreads), 0, st, part, nb,
                       dice_scale(n, c, loss_weight, avg_factor), loss);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

extern "C" int seg3d_dice_loss_bwd(const float* logits, const int64_t* labels, const float* grad_out, int64_t n, int32_t c,
                                   int64_t ignore_index, float smooth, float exponent, const float* class_weight,
                                   float loss_weight, float avg_factor, float* dlogits, void* stream) {
    DiceArgs a;
    if (n < 0 || !dice_args(c, ignore_index, smooth, exponent, &a) || !grad_out) return SEG3D_EINVAL;
    if (n == 0) return SEG3D_OK;
    if (!logits || !labels || !dlogits) return SEG3D_EINVAL;
    hipLaunchKernelGGL(dice_bwd_kernel, dim3((unsigned)dice_blocks(n)), dim3(kDiceRows),
                       (size_t)kDiceRows * (c | 1) * sizeof(float), as_stream(stream), logits, labels, grad_out, n, a,
                       class_weight, (float)dice_scale(n, c, loss_weight, avg_factor), dlogits);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}
