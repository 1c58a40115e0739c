// Optimizer step: SGD (momentum) and AdamW over every parameter tensor of a model in one launch.
// A pure stream: per element 3 reads + 2 writes (SGD with momentum, 20 B) or 4 reads + 3 writes (AdamW, 28 B); no
// atomics, no LDS.  The arithmetic is optim_update.hpp's, shared with the host twin at the bottom of this file.
// Beside the step, on the same table and grid: the global L2 norm of the gradients summed in fp64, and the clip by it
// (seg3d_grad_norm / seg3d_grad_scale).
#include "common.hpp"
#include "optim_update.hpp"
#include "wave_ops.hpp"

static_assert(sizeof(seg3d_optim_tensor) == 64, "seg3d_optim_tensor layout is part of the C ABI (seg3d_optim_step)");
static_assert(sizeof(seg3d_optim_hyper) == 32, "seg3d_optim_hyper layout is part of the C ABI (seg3d_optim_step)");

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                            // 16-byte vectors per thread and array
constexpr int kBlockElems = kThreads * 4 * kUnroll;  // 4096 elements = 16 KB per array and workgroup

typedef float vec4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vec4 gvec;

// the hyper-parameter sets travel in the kernel arguments: new values every step without an upload
struct HyperArgs {
    seg3d_optim_hyper s[SEG3D_OPTIM_MAX_HYPER];
};

template <int ALGO>
__host__ __device__ inline void update_at(float* p, const float* g, float* s0, float* s1, int64_t i, bool first,
                                          const seg3d_optim_hyper* h) {
    if (ALGO == SEG3D_OPTIM_SGD) sgd_update(p + i, g[i], s0 ? s0 + i : nullptr, first, h);
    else adamw_update(p + i, g[i], s0 + i, s1 + i, h);
}

// one 16-byte vector of each array, already in registers
template <int ALGO>
__device__ __forceinline__ void update_vec(vec4* p, const vec4& g, vec4* s0, vec4* s1, bool has_s0, bool first,
                                           const seg3d_optim_hyper* h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = (*p)[j], aj = (*s0)[j], bj = (*s1)[j];
        if (ALGO == SEG3D_OPTIM_SGD) sgd_update(&pj, g[j], has_s0 ? &aj : nullptr, first, h);
        else adamw_update(&pj, g[j], &aj, &bj, h);
        (*p)[j] = pj;
        (*s0)[j] = aj;
        (*s1)[j] = bj;
    }
}

template <int ALGO>
__global__ __launch_bounds__(kThreads) void optim_step_kernel(const seg3d_optim_tensor* __restrict__ table, int n_tensors,
                                                               HyperArgs hyper, int n_hyper) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {  // last tensor with first_block <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= (int64_t)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const seg3d_optim_tensor r = table[lo];
    if ((unsigned)r.hyper >= (unsigned)n_hyper) return;
    const int64_t start = ((int64_t)blockIdx.x - r.first_block) * kBlockElems;
    if (start < 0 || start >= r.count) return;
    const seg3d_optim_hyper h = hyper.s[r.hyper];
    const int n_here = (int)(r.count - start < kBlockElems ? r.count - start : kBlockElems);
    const bool first = (r.flags & SEG3D_OPTIM_FIRST_STEP) != 0;
    const bool has_s0 = ALGO == SEG3D_OPTIM_ADAMW || r.state0 != nullptr;
    float* p = r.param + start;
    const float* g = r.grad + start;
    float* s0 = has_s0 ? r.state0 + start : nullptr;
    float* s1 = ALGO == SEG3D_OPTIM_ADAMW ? r.state1 + start : nullptr;
    const int tid = threadIdx.x;
    // start is a multiple of 4096 elements: the chunk is aligned when the tensor's pointers are
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0;
    if (!aligned) {  // gradient views into a flat arena sit at any 4-byte offset
        for (int i = tid; i < n_here; i += kThreads) update_at<ALGO>(p, g, s0, s1, i, first, &h);
        return;
    }
    // the pointers come out of a record in memory: say that they are global, or the loads and stores are flat ones
    gvec* p4 = (gvec*)p;
    const gvec* g4 = (const gvec*)g;
    gvec* a4 = (gvec*)s0;
    gvec* b4 = (gvec*)s1;
    if (n_here == kBlockElems) {  // a full chunk: every load issued before the first use
        vec4 pv[kUnroll], gv[kUnroll], av[kUnroll] = {}, bv[kUnroll] = {};
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int v = u * kThreads + tid;
            pv[u] = p4[v];
            gv[u] = g4[v];
            if (has_s0) av[u] = a4[v];
            if (ALGO == SEG3D_OPTIM_ADAMW) bv[u] = b4[v];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int v = u * kThreads + tid;
            update_vec<ALGO>(&pv[u], gv[u], &av[u], &bv[u], has_s0, first, &h);
            p4[v] = pv[u];
            if (has_s0) a4[v] = av[u];
            if (ALGO == SEG3D_OPTIM_ADAMW) b4[v] = bv[u];
        }
        return;
    }
    const int n_vec = n_here >> 2;
    for (int v = tid; v < n_vec; v += kThreads) {
        vec4 pv = p4[v], av = {}, bv = {};
        const vec4 gv = g4[v];
        if (has_s0) av = a4[v];
        if (ALGO == SEG3D_OPTIM_ADAMW) bv = b4[v];
        update_vec<ALGO>(&pv, gv, &av, &bv, has_s0, first, &h);
        p4[v] = pv;
        if (has_s0) a4[v] = av;
        if (ALGO == SEG3D_OPTIM_ADAMW) b4[v] = bv;
    }
    const int i = n_vec * 4 + tid;  // the last count % 4 elements
    if (i < n_here) update_at<ALGO>(p, g, s0, s1, i, first, &h);
}

int check_call(const void* table, int32_t n_tensors, int64_t total_blocks, const void* hyper, int32_t n_hyper,
               int32_t algo) {
    if (algo != SEG3D_OPTIM_SGD && algo != SEG3D_OPTIM_ADAMW) return SEG3D_EINVAL;
    if (n_tensors < 0 || n_hyper < 0 || n_hyper > SEG3D_OPTIM_MAX_HYPER) return SEG3D_EINVAL;
    if (total_blocks < 0 || total_blocks > 0x7FFFFFFF) return SEG3D_EINVAL;
    if (n_tensors > 0 && (!table || n_hyper == 0)) return SEG3D_EINVAL;
    if (n_hyper > 0 && !hyper) return SEG3D_EINVAL;
    return SEG3D_OK;
}

template <int ALGO>
void host_step(const seg3d_optim_tensor* table, int32_t n_tensors, const seg3d_optim_hyper* hyper) {
    for (int32_t t = 0; t < n_tensors; ++t) {
        const seg3d_optim_tensor& r = table[t];
        const bool first = (r.flags & SEG3D_OPTIM_FIRST_STEP) != 0;
        for (int64_t i = 0; i < r.count; ++i) update_at<ALGO>(r.param, r.grad, r.state0, r.state1, i, first, &hyper[r.hyper]);
    }
}

// ---------------------------------------------------------------- gradient-norm clipping
// The same table and grid as the step; record.param is the gradient array.  Norm: one fp64 partial per workgroup, then one
// workgroup over the partials; scale: g = g * coef unless the coefficient is 1.  No atomics: the same bits on every run.
typedef __attribute__((address_space(1))) float gfloat;

// last tensor with first_block <= blockIdx.x (the bisection of optim_step_kernel)
__device__ __forceinline__ int tensor_of_block(const seg3d_optim_tensor* __restrict__ table, int n_tensors) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= (int64_t)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__host__ __device__ inline double square64(float g) {  // exact: 24 x 24 significand bits, and no float32 range limit
    const double d = (double)g;
    return d * d;
}

// {norm, clip coefficient} from the sum of squares: torch's max_norm / (total_norm + 1e-6) clamped at 1, in float32
__host__ __device__ inline void norm_result(double total, float max_norm, bool nothing, float* result) {
    const float norm = (float)sqrt(total);
    float c = max_norm / (norm + 1e-6f);
    if (c > 1.0f || nothing) c = 1.0f;  // a NaN c stays NaN
    result[0] = norm;
    result[1] = c;
}

__global__ __launch_bounds__(kThreads) void grad_norm_partial_kernel(const seg3d_optim_tensor* __restrict__ table,
                                                                      int n_tensors, double* __restrict__ partials) {
    const seg3d_optim_tensor r = table[tensor_of_block(table, n_tensors)];
    const int64_t start = ((int64_t)blockIdx.x - r.first_block) * kBlockElems;
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (start >= 0 && start < r.count) {  // (no early return: every thread reaches the workgroup sum)
        const int n_here = (int)(r.count - start < kBlockElems ? r.count - start : kBlockElems);
        const float* g = r.param + start;
        if (((uintptr_t)g & 15) != 0) {  // a gradient view at a 4-byte offset
            const gfloat* g1 = (const gfloat*)g;
            for (int i = tid; i < n_here; i += kThreads) acc += square64(g1[i]);
        } else {
            const gvec* g4 = (const gvec*)g;
            if (n_here == kBlockElems) {  // a full chunk: every load issued before the first use
                vec4 gv[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) gv[u] = g4[u * kThreads + tid];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc += square64(gv[u][j]);
            } else {
                const int n_vec = n_here >> 2;
                for (int v = tid; v < n_vec; v += kThreads) {
                    const vec4 gv = g4[v];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc += square64(gv[j]);
                }
                const int i = n_vec * 4 + tid;  // the last count % 4 elements
                if (i < n_here) acc += square64(((const gfloat*)g)[i]);
            }
        }
    }
    const double total = block_sum<kThreads, double>(acc);
    if (tid == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void grad_norm_final_kernel(const double* __restrict__ partials, int n_partials,
                                                                    float max_norm, float* __restrict__ result) {
    // thread t adds partials t, t + 256, ... in ascending order; 16 loads are in flight before the first add (one load
    // per add: 9.4 us for the model's 8041 partials, all of it latency).  Past the end a +0.0 is added: the same bits.
    constexpr int kBatch = 16;
    double acc = 0.0;
    for (int64_t base = threadIdx.x; base < n_partials; base += (int64_t)kBatch * kThreads) {
        double v[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int64_t i = base + (int64_t)u * kThreads;
            v[u] = i < n_partials ? partials[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) acc += v[u];
    }
    const double total = block_sum<kThreads, double>(acc);
    if (threadIdx.x == 0) norm_result(total, max_norm, n_partials == 0, result);
}

__global__ __launch_bounds__(kThreads) void grad_scale_kernel(const seg3d_optim_tensor* __restrict__ table, int n_tensors,
                                                               const float* __restrict__ coef) {
    const float c = *coef;
    if (c == 1.0f) return;  // the healthy run: nothing is read or written (a NaN coefficient is not 1)
    const seg3d_optim_tensor r = table[tensor_of_block(table, n_tensors)];
    const int64_t start = ((int64_t)blockIdx.x - r.first_block) * kBlockElems;
    if (start < 0 || start >= r.count) return;
    const int n_here = (int)(r.count - start < kBlockElems ? r.count - start : kBlockElems);
    float* g = r.param + start;
    const int tid = threadIdx.x;
    if (((uintptr_t)g & 15) != 0) {
        gfloat* g1 = (gfloat*)g;
        for (int i = tid; i < n_here; i += kThreads) g1[i] = g1[i] * c;
        return;
    }
    gvec* g4 = (gvec*)g;
    if (n_here == kBlockElems) {
        vec4 gv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) gv[u] = g4[u * kThreads + tid];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) g4[u * kThreads + tid] = gv[u] * c;
        return;
    }
    const int n_vec = n_here >> 2;
    for (int v = tid; v < n_vec; v += kThreads) {
        const vec4 gv = g4[v];
        g4[v] = gv * c;
    }
    const int i = n_vec * 4 + tid;
    if (i < n_here) ((gfloat*)g)[i] = ((gfloat*)g)[i] * c;
}

int check_grad_call(const void* table, int32_t n_tensors, int64_t total_blocks) {
    if (n_tensors < 0 || total_blocks < 0 || total_blocks > 0x7FFFFFFF) return SEG3D_EINVAL;
    if (n_tensors > 0 && !table) return SEG3D_EINVAL;
    return SEG3D_OK;
}

// what the device entries cannot do: read the table
int check_grad_records(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks) {
    int64_t next_block = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        const seg3d_optim_tensor& r = table[t];
        if (r.count < 0 || r.first_block != next_block || (r.count > 0 && !r.param)) return SEG3D_EINVAL;
        next_block += ceil_div64(r.count, kBlockElems);
    }
    return next_block == total_blocks ? SEG3D_OK : SEG3D_EINVAL;
}

}  // namespace

extern "C" {

int32_t seg3d_optim_block_elems(void) { return kBlockElems; }

size_t seg3d_grad_norm_workspace_bytes(int64_t total_blocks) {
    return total_blocks > 0 ? (size_t)total_blocks * sizeof(double) : 0;
}

int seg3d_grad_norm(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, float max_norm,
                    void* workspace, size_t workspace_bytes, float* result, void* stream) {
    if (const int rc = check_grad_call(table, n_tensors, total_blocks); rc != SEG3D_OK) return rc;
    if (!result || !(max_norm >= 0.0f)) return SEG3D_EINVAL;  // (a NaN max_norm fails the comparison)
    const bool nothing = n_tensors == 0 || total_blocks == 0;
    if (!nothing) {
        if (!workspace) return SEG3D_EINVAL;
        if (workspace_bytes < seg3d_grad_norm_workspace_bytes(total_blocks)) return SEG3D_EWORKSPACE;
        hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)total_blocks), dim3(kThreads), 0, as_stream(stream),
                           table, (int)n_tensors, (double*)workspace);
        SEG3D_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), (const double*)workspace,
                       nothing ? 0 : (int)total_blocks, max_norm, result);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_grad_scale(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, const float* coef,
                     void* stream) {
    if (const int rc = check_grad_call(table, n_tensors, total_blocks); rc != SEG3D_OK) return rc;
    if (!coef) return SEG3D_EINVAL;
    if (n_tensors == 0 || total_blocks == 0) return SEG3D_OK;
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)total_blocks), dim3(kThreads), 0, as_stream(stream), table,
                       (int)n_tensors, coef);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

int seg3d_grad_norm_host(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, float max_norm,
                         float* result) {
    if (const int rc = check_grad_call(table, n_tensors, total_blocks); rc != SEG3D_OK) return rc;
    if (!result || !(max_norm >= 0.0f)) return SEG3D_EINVAL;
    if (n_tensors > 0)
        if (const int rc = check_grad_records(table, n_tensors, total_blocks); rc != SEG3D_OK) return rc;
    double total = 0.0;
    for (int32_t t = 0; t < n_tensors; ++t)
        for (int64_t i = 0; i < table[t].count; ++i) total += square64(table[t].param[i]);
    norm_result(total, max_norm, n_tensors == 0 || total_blocks == 0, result);
    return SEG3D_OK;
}

int seg3d_grad_scale_host(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks, const float* coef) {
    if (const int rc = check_grad_call(table, n_tensors, total_blocks); rc != SEG3D_OK) return rc;
    if (!coef) return SEG3D_EINVAL;
    if (n_tensors == 0) return SEG3D_OK;
    if (const int rc = check_grad_records(table, n_tensors, total_blocks); rc != SEG3D_OK) return rc;
    const float c = *coef;
    if (c == 1.0f) return SEG3D_OK;
    for (int32_t t = 0; t < n_tensors; ++t)
        for (int64_t i = 0; i < table[t].count; ++i) table[t].param[i] = table[t].param[i] * c;
    return SEG3D_OK;
}

int seg3d_optim_step(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks,
                     const seg3d_optim_hyper* hyper, int32_t n_hyper, int32_t algo, void* stream) {
    if (const int rc = check_call(table, n_tensors, total_blocks, hyper, n_hyper, algo); rc != SEG3D_OK) return rc;
    if (n_tensors == 0 || total_blocks == 0) return SEG3D_OK;
    HyperArgs args = {};
    for (int i = 0; i < n_hyper; ++i) args.s[i] = hyper[i];
    if (algo == SEG3D_OPTIM_SGD)
        hipLaunchKernelGGL(optim_step_kernel<SEG3D_OPTIM_SGD>, dim3((unsigned)total_blocks), dim3(kThreads), 0,
                           as_stream(stream), table, (int)n_tensors, args, (int)n_hyper);
    else
        hipLaunchKernelGGL(optim_step_kernel<SEG3D_OPTIM_ADAMW>, dim3((unsigned)total_blocks), dim3(kThreads), 0,
                           as_stream(stream), table, (int)n_tensors, args, (int)n_hyper);
    SEG3D_CHECK_LAUNCH();
    return SEG3D_OK;
}

// The same table with host pointers, plain C++: the reference the device entry is tested against, bit for bit, and the
// step of parameters that live on the CPU.
int seg3d_optim_step_host(const seg3d_optim_tensor* table, int32_t n_tensors, int64_t total_blocks,
                          const seg3d_optim_hyper* hyper, int32_t n_hyper, int32_t algo) {
    if (const int rc = check_call(table, n_tensors, total_blocks, hyper, n_hyper, algo); rc != SEG3D_OK) return rc;
    if (n_tensors == 0) return SEG3D_OK;
    int64_t next_block = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        const seg3d_optim_tensor& r = table[t];
        if (r.count < 0 || r.hyper < 0 || r.hyper >= n_hyper || r.first_block != next_block) return SEG3D_EINVAL;
        if (r.count > 0 && (!r.param || !r.grad)) return SEG3D_EINVAL;
        if (r.count > 0 && algo == SEG3D_OPTIM_ADAMW && (!r.state0 || !r.state1)) return SEG3D_EINVAL;
        next_block += ceil_div64(r.count, kBlockElems);
    }
    if (next_block != total_blocks) return SEG3D_EINVAL;
    if (algo == SEG3D_OPTIM_SGD) host_step<SEG3D_OPTIM_SGD>(table, n_tensors, hyper);
    else host_step<SEG3D_OPTIM_ADAMW>(table, n_tensors, hyper);
    return SEG3D_OK;
}

}  // extern "C"
