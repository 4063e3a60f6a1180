// The total order of a logits row that token_sample.hip, beam_search.hip and contrastive.hip share: value descending, then index ascending; NaN above +inf above
// the finite values above -inf; -0 ties with +0.  Every element gets a monotone integer key of its STORED value (16 bits for bf16, 32 for fp32;
// all NaNs share the top key), so ties are exactly the input's.  With the 8-element row loads and the 64-bit wavefront reductions these files use.
#pragma once
#include "common.h"

#include <float.h>

namespace {

typedef unsigned long long u64;

template <class T> struct KeyBits;
template <> struct KeyBits<float> { static constexpr int value = 32; };
template <> struct KeyBits<bf16_t> { static constexpr int value = 16; };

// monotone key of the stored value: larger key = earlier in the order
template <int KB> __device__ __forceinline__ uint32_t key_of(float x) {
    if (x != x) return 0xFFFFFFFFu >> (32 - KB);
    uint32_t b = x == 0.f ? 0u : __float_as_uint(x);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return b >> (32 - KB);
}

// the value of a key (not the NaN key)
template <int KB> __device__ __forceinline__ float value_of(uint32_t key) {
    uint32_t b = key << (32 - KB);
    if (!(b & 0x80000000u)) b |= (uint32_t)((1ull << (32 - KB)) - 1);
    b = (b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b;
    return __uint_as_float(b);
}

template <int KB> __device__ __forceinline__ bool key_finite(uint32_t key) {
    return key != (0xFFFFFFFFu >> (32 - KB)) && fabsf(value_of<KB>(key)) <= FLT_MAX;
}

// elements i0 .. i0 + 7 of a row as floats; returns how many lie below V.  vec: the row base is 16-byte aligned (i0 is a multiple of 8)
__device__ __forceinline__ int load8(const bf16_t* __restrict__ row, int i0, int V, bool vec, float (&x)[8]) {
    const int n = V - i0 >= 8 ? 8 : V - i0 > 0 ? V - i0 : 0;
    if (vec && n == 8) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + i0);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[2 * j] = __uint_as_float(w[j] << 16);
            x[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = j < n ? (float)row[i0 + j] : 0.f;
    }
    return n;
}

__device__ __forceinline__ int load8(const float* __restrict__ row, int i0, int V, bool vec, float (&x)[8]) {
    const int n = V - i0 >= 8 ? 8 : V - i0 > 0 ? V - i0 : 0;
    if (vec && n == 8) {
        const float4 a = *reinterpret_cast<const float4*>(row + i0), b = *reinterpret_cast<const float4*>(row + i0 + 4);
        x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = j < n ? row[i0 + j] : 0.f;
    }
    return n;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const u64 o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// (key, index) as one integer whose order is the row's: the larger key first, then the lower index.  Every key of an element is > 0
__device__ __forceinline__ u64 pack_top(uint32_t key, int idx) { return ((u64)key << 32) | (u64)(0xFFFFFFFFu - (uint32_t)idx); }

}  // namespace
