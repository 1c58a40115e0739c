// The recipes the instance bank is built with (instance_extract.hip) and pasted from (augment_instance.hip): how a label
// is read, how distances are formed and compared, and the ONE summation order of a mean, on the device and in the host
// twins.  A centre or radius computed by one file is consumed by the other, so both take these from here; a different
// order of the sums or a fused multiply-add in either would move the bits.  Workgroups are kThreads wide.
#pragma once
#include <math.h>

#include <vector>

#include "common.hpp"

// fixed sequences of IEEE products and sums, as numpy rounds them; no fused multiply-add (see augment.hip)
#pragma clang fp contract(off)

namespace {  // internal to each of the two files, like the rest of their helpers

constexpr int kThreads = 256;

// labels are uint8 (label_bytes == 1) or int64
__host__ __device__ __forceinline__ int64_t label_at(const void* labels, int label_bytes, int64_t i) {
    return label_bytes == 1 ? (int64_t) static_cast<const uint8_t*>(labels)[i] : static_cast<const int64_t*>(labels)[i];
}

// (distance, row) ordered lexicographically: np.argmin keeps the lowest index among equal distances
__host__ __device__ __forceinline__ bool closer(double d, int32_t row, double bd, int32_t brow) {
    return d < bd || (d == bd && row < brow);
}

// np.linalg.norm over three columns: ((dx*dx + dy*dy) + dz*dz), IEEE sqrt
__host__ __device__ __forceinline__ double dist3(double x, double y, double z, const double* c) {
    const double dx = x - c[0], dy = y - c[1], dz = z - c[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// The fixed summation order of a mean: thread t adds rows t, t + 256, ... in ascending order (the caller's loop), then
// the 256 partial sums are folded by halving (t += t + 128, t += t + 64, ...).  lds holds 3 * kThreads doubles; the sums
// come back in every thread.  sum3_host below does the same.
__device__ void block_sum3(double* v, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int c = 0; c < 3; ++c) lds[c * kThreads + t] = v[c];
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int c = 0; c < 3; ++c) lds[c * kThreads + t] += lds[c * kThreads + t + s];
        __syncthreads();
    }
    for (int c = 0; c < 3; ++c) v[c] = lds[c * kThreads];
}

__device__ double block_max(double v, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s && lds[t + s] > lds[t]) lds[t] = lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

void sum3_host(const std::vector<double>& part, double* v) {  // part [3][kThreads]: block_sum3's fold
    std::vector<double> l(part);
    for (int s = kThreads / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t)
            for (int c = 0; c < 3; ++c) l[c * kThreads + t] += l[c * kThreads + t + s];
    for (int c = 0; c < 3; ++c) v[c] = l[c * kThreads];
}

}  // namespace
