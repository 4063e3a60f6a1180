// Helpers shared by the deformable-sampling files (dcnv3.hip, defattn.hip): raw 16-byte row unpacking, the 2^-40 int64 fixed-point conversion behind
// every order-free input-gradient accumulator, and the zero / unfix / flag passes around it.  Everything is TU-local (anonymous namespace).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void unpack_raw_bf16x8(const uint4& r, float* v) {
    v[0] = __uint_as_float(r.x << 16), v[1] = __uint_as_float(r.x & 0xffff0000u);
    v[2] = __uint_as_float(r.y << 16), v[3] = __uint_as_float(r.y & 0xffff0000u);
    v[4] = __uint_as_float(r.z << 16), v[5] = __uint_as_float(r.z & 0xffff0000u);
    v[6] = __uint_as_float(r.w << 16), v[7] = __uint_as_float(r.w & 0xffff0000u);
}

template <class T, int CG> __device__ __forceinline__ void dcn_unpack_row(const uint4* raw, float* v) {
    constexpr int RAW = CG * (int)sizeof(T) / 16;
#pragma unroll
    for (int r = 0; r < RAW; ++r) {
        if constexpr (sizeof(T) == 2) unpack_raw_bf16x8(raw[r], v + r * 8);
        else {
            v[r * 4] = __uint_as_float(raw[r].x), v[r * 4 + 1] = __uint_as_float(raw[r].y);
            v[r * 4 + 2] = __uint_as_float(raw[r].z), v[r * 4 + 3] = __uint_as_float(raw[r].w);
        }
    }
}

// 2^-40 fixed point (int64) for every input-gradient accumulator of these files: integer adds commute, so atomics give the same bits whatever
// the order (the reference's default is a deterministic step, core_env.py:39-48).  |v| < 2^23, resolution 9.1e-13.
constexpr float DCN_FIX = 256.f;                  // 2^8: high word = floor(v * 2^8), low word = fract * 2^32
constexpr double DCN_UNFIX = 1.0 / 1099511627776.0;      // 2^-40
// Sign and magnitude: the magnitude's integer part and fraction are both exact in fp32 (a - floor(a) of a non-negative a needs no more bits than
// a has), so the only error is the rounding at 2^-40.  (Rounds 4-5 split the SIGNED value: floor(v) = -1 for a small negative v and the
// fraction v + 1 was rounded to fp32's 2^-24 next to 1 -- a resolution of 2^-32 = 2.3e-10 instead of 9.1e-13 for every negative contribution,
// which the 512 x 512 parity of round 6 found: gradient elements of 1e-9 under a mean loss over 262 144 pixels were off by per cent.)
__device__ __forceinline__ unsigned long long dcn_to_fixed(float v256) {      // v256 = value * 2^8
    const float a = fabsf(v256);
    const float fl = floorf(a);
    const unsigned hi = (unsigned)(int)fl;                      // (int): saturating
    const unsigned lo = (unsigned)rintf((a - fl) * 4294967296.f);      // nearest (truncation shrinks every contribution: a bias; 2^32 saturates one quantum low)
    const unsigned long long mag = ((unsigned long long)hi << 32) | lo;
    return v256 < 0.f ? 0ull - mag : mag;
}

__global__ void dcn_flag_reset_kernel(int* __restrict__ flag) { *flag = 0; }

// flag (may be null): bit 1 set by an accumulating kernel that met a non-finite contribution -- the fixed-point conversion saturates those to finite
// garbage, so the whole input gradient is written as NaN instead (what a chain of fp32 atomics would have spread; the window route does the same)
template <class TO>
__global__ __launch_bounds__(256) void dcn_unfix_kernel(const unsigned long long* __restrict__ acc, TO* __restrict__ dx, int64_t n,
                                                        const int* __restrict__ flag = nullptr) {
    const bool poisoned = flag != nullptr && (*flag & 2) != 0;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dx[i] = from_f32<TO>(poisoned ? __builtin_nanf("") : (float)((double)(long long)acc[i] * DCN_UNFIX));
}

__global__ __launch_bounds__(256) void dcn_zero_kernel(uint4* __restrict__ p, int64_t n16) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

static inline unsigned lane_blocks(int64_t n) { return grid_cap(n, 256, 256 * 64); }

}  // namespace
