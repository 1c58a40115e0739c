// Optimizer step: SGD (momentum) and AdamW over every parameter tensor of a model in one launch.
// A pure stream: per element 3 reads + 2 writes (SGD with momentum, 20 B) or 4 reads + 3 writes (AdamW, 28 B); no
// atomics, no LDS.  The arithmetic is optim_update.hpp's, shared with the host twin at the bottom of this file.
#include "common.hpp"
#include "optim_update.hpp"

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

}  // namespace

extern "C" {

int32_t seg3d_optim_block_elems(void) { return kBlockElems; }

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
