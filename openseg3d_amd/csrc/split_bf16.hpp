// The split-bf16 arithmetic of every MFMA kernel -- its only definition.
//
// Contract.  An fp32 operand x becomes hi = RNE(x), lo = RNE(x - hi): round-to-nearest-even at EVERY level, never
// truncation (x - hi is exact in fp32; 16 significant bits survive).  A product a . b is three v_mfma_f32_16x16x32_bf16
// into one fp32 accumulator, issued lo*hi, hi*lo, hi*hi (mfma3); the lo*lo term (<= 2^-18 of the product) is dropped.
// When b IS bf16 it is its own high half: two MFMAs, lo*b then hi*b (mfma2), nothing dropped on b's side.  The three-way
// split x = h + m + l (split3) is exact; linear_x6.hip takes the six products down to 2^-16 of the leading one and
// drops m*l, l*m, l*l.  fp32 addition does not associate: the ORDER of the MFMAs is part of the result's bits, and the
// bit-identity tests between kernel families rest on every kernel taking these bodies unchanged.
#pragma once
#include "common.hpp"

namespace sbf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// operands of ds_read_b64_tr_b16 (transposed LDS fragment reads)
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ void split1(float v, __bf16* hi, __bf16* lo) {
    const __bf16 h = (__bf16)v;
    *hi = h;
    *lo = (__bf16)(v - (float)h);
}

// two fp32 -> packed bf16 hi pair and lo pair
__device__ __forceinline__ void split2(float a, float b, uint32_t* hi, uint32_t* lo) {
    const uint32_t w = pack_bf16(a, b);
    *hi = w;
    *lo = pack_bf16(a - __builtin_bit_cast(float, w << 16), b - __builtin_bit_cast(float, w & 0xFFFF0000u));
}

// 8 floats -> (hi, lo) bf16 MFMA fragments; hi = RNE(x), lo = RNE(x - hi).  One body, as packed dwords; the other
// signatures forward to it.
__device__ __forceinline__ void split_frag(const float* v, u32x4* hi, u32x4* lo) {
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = pack_bf16(v[2 * i], v[2 * i + 1]);
        const float h0 = __builtin_bit_cast(float, w << 16);
        const float h1 = __builtin_bit_cast(float, w & 0xFFFF0000u);
        h[i] = w;
        l[i] = pack_bf16(v[2 * i] - h0, v[2 * i + 1] - h1);
    }
    *hi = h;
    *lo = l;
}
__device__ __forceinline__ void split_frag(const float* v, bf16x8* hi, bf16x8* lo) {
    u32x4 h, l;
    split_frag(v, &h, &l);
    *hi = __builtin_bit_cast(bf16x8, h);
    *lo = __builtin_bit_cast(bf16x8, l);
}
__device__ __forceinline__ void split8(const f32x4& p, const f32x4& q, u32x4* hi, u32x4* lo) {
    const float v[8] = {p[0], p[1], p[2], p[3], q[0], q[1], q[2], q[3]};
    split_frag(v, hi, lo);
}
__device__ __forceinline__ void split8(const f32x4& p, const f32x4& q, bf16x8* hi, bf16x8* lo) {
    const float v[8] = {p[0], p[1], p[2], p[3], q[0], q[1], q[2], q[3]};
    split_frag(v, hi, lo);
}

// the same from four float pairs: the low halves come out of one packed subtract per pair (v_pk_add_f32)
__device__ __forceinline__ void split_frag2(const f32x2* v, bf16x8* hi, bf16x8* lo) {
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = pack_bf16(v[i][0], v[i][1]);
        const f32x2 hf = {__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xFFFF0000u)};
        const f32x2 d = v[i] - hf;
        h[i] = w;
        l[i] = pack_bf16(d[0], d[1]);
    }
    *hi = __builtin_bit_cast(bf16x8, h);
    *lo = __builtin_bit_cast(bf16x8, l);
}

// 8 fp32 -> three bf16 fragments with h + m + l == x exactly (round-to-nearest at every level; |m| <= 2^-9 |x|, |l| <= 2^-18 |x|)
__device__ __forceinline__ void split3(const float* v, bf16x8* h, bf16x8* m, bf16x8* l) {
    u32x4 H, M, L;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t wh = pack_bf16(v[2 * i], v[2 * i + 1]);
        const float r0 = v[2 * i] - __builtin_bit_cast(float, wh << 16);
        const float r1 = v[2 * i + 1] - __builtin_bit_cast(float, wh & 0xFFFF0000u);
        const uint32_t wm = pack_bf16(r0, r1);
        const float s0 = r0 - __builtin_bit_cast(float, wm << 16);
        const float s1 = r1 - __builtin_bit_cast(float, wm & 0xFFFF0000u);
        H[i] = wh;
        M[i] = wm;
        L[i] = pack_bf16(s0, s1);
    }
    *h = __builtin_bit_cast(bf16x8, H);
    *m = __builtin_bit_cast(bf16x8, M);
    *l = __builtin_bit_cast(bf16x8, L);
}

// acc += a . b in split-bf16 (hi*hi + hi*lo + lo*hi)
__device__ __forceinline__ f32x4 mfma3(const bf16x8& a_hi, const bf16x8& a_lo, const bf16x8& b_hi, const bf16x8& b_lo,
                                       f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b_hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_hi, acc, 0, 0, 0);
    return acc;
}

// acc += a . b for a split-bf16 `a` and a `b` that IS bf16 (a bf16 row is its own high half: no a_hi * b_lo term)
__device__ __forceinline__ f32x4 mfma2(const bf16x8& a_hi, const bf16x8& a_lo, const bf16x8& b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b, acc, 0, 0, 0);
    return acc;
}

// bf16 fragment of channel `comp` (0..3) of a lane's quad from 8 rows of 4 bf16 each (q[i] = row i: {ch0 | ch1 << 16, ch2 | ch3 << 16})
__device__ __forceinline__ bf16x8 frag_from_bf16_rows(const uint2* q, int comp) {
    u32x4 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t a = (comp & 2) ? q[2 * j].y : q[2 * j].x, b = (comp & 2) ? q[2 * j + 1].y : q[2 * j + 1].x;
        h[j] = (comp & 1) ? ((a >> 16) | (b & 0xFFFF0000u)) : ((a & 0xFFFFu) | (b << 16));
    }
    return __builtin_bit_cast(bf16x8, h);
}

// 16-B fragment load (8 bf16) from a hi block and the lo block `half` elements behind it; zero when !ok
__device__ __forceinline__ void load_frag(const __bf16* base, int64_t off, int64_t half, bool ok, bf16x8* hi, bf16x8* lo) {
    u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
    if (ok) {
        a = *reinterpret_cast<const u32x4*>(base + off);
        b = *reinterpret_cast<const u32x4*>(base + half + off);
    }
    *hi = __builtin_bit_cast(bf16x8, a);
    *lo = __builtin_bit_cast(bf16x8, b);
}

}  // namespace sbf
