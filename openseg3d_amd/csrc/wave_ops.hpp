// Fixed-order sums and scans over a wave64 and over a workgroup.  fp32 and fp64 sums do not associate, and the fused
// criterion returns the bits of the per-term entries, the device the bits of its host twins: every caller that wants
// "the sum over the workgroup" takes THESE operations in THIS order.  Reductions of another shape (16-lane groups,
// runtime widths, minima) stay where they are; tests/test_csrc_layout.py lists them.
#pragma once
#include "common.hpp"

// sum over the wave, in every lane: xor tree, offsets 32 ... 1
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, SEG3D_WAVE);
    return v;
}

// ... of two values, level by level together
template <typename T>
__device__ __forceinline__ void wave_sum(T& a, T& b) {
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, SEG3D_WAVE);
        b += __shfl_xor(b, off, SEG3D_WAVE);
    }
}

// inclusive prefix sum over the lanes of the wave: __shfl_up, offsets 1 ... 32
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, SEG3D_WAVE);
        if (lane >= off) v += o;
    }
    return v;
}

// Sum over a workgroup of THREADS threads (all of them call it): wave_sum, then thread 0 adds the waves' sums to 0 in
// ascending order.  The result is valid in thread 0 ONLY.  The LDS is the instantiation's own: two calls of one
// <THREADS, T> need a barrier between them.
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v) {
    __shared__ T red[THREADS / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / 64; ++w) t += red[w];
    return t;
}

// ... of two values at once (one barrier); a and b are replaced in thread 0 only
template <int THREADS, typename T>
__device__ __forceinline__ void block_sum(T& a, T& b) {
    __shared__ T red[2][THREADS / 64];
    wave_sum(a, b);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        T sa = 0, sb = 0;
        for (int w = 0; w < THREADS / 64; ++w) {
            sa += red[0][w];
            sb += red[1][w];
        }
        a = sa;
        b = sb;
    }
}

// inclusive prefix sum of v over the workgroup's threads, and the total, in every thread
template <int THREADS, typename T>
__device__ __forceinline__ T block_scan_inclusive(T v, T* total) {
    __shared__ T wsum[THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = wave_scan_inclusive(v, lane);
    __syncthreads();  // wsum may still be read from an earlier call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T t = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
        if (w < wave) inc += wsum[w];
        t += wsum[w];
    }
    *total = t;
    return inc;
}
