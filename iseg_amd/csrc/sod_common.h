// Helpers shared by the salient-object-detection kernels (sod_metrics.hip, sod_fmv2.hip): prepare_data's fp32 normalisation
// (metrics/sod/sod_metric_utils.py:82-95 of the reference), the pixel loads and the wave64 butterflies.
#pragma once
#include "common.h"

namespace {

struct NormP {
    float mn, den;
    int on;
};

// mapminmax parameters from the grey-level extrema of a uint8 prediction (normalize = 0: the identity)
__device__ __forceinline__ NormP norm_from_minmax(int umin, int umax, int normalize) {
    NormP n{0.f, 1.f, 0};
    if (normalize) {
        const float fmn = __fdiv_rn((float)umin, 255.f), fmx = __fdiv_rn((float)umax, 255.f);
        n.mn = fmn;
        n.den = fmx - fmn;
        n.on = umax != umin;
    }
    return n;
}
// im2double then mapminmax, in the reference's fp32 operation order
__device__ __forceinline__ float norm_u8(unsigned u, const NormP& n) {
    const float v = __fdiv_rn((float)u, 255.f);
    return n.on ? __fdiv_rn(v - n.mn, n.den) : v;
}
template <bool U8> __device__ __forceinline__ float load_p(const void* pred, int64_t i, const NormP& n) {
    if (U8) return norm_u8(reinterpret_cast<const uint8_t*>(pred)[i], n);
    return reinterpret_cast<const float*>(pred)[i];
}
template <bool U8> __device__ __forceinline__ void load_p4(const void* pred, int64_t i, const NormP& n, float* p) {
    if (U8) {
        const uchar4 u = *reinterpret_cast<const uchar4*>(reinterpret_cast<const uint8_t*>(pred) + i);
        p[0] = norm_u8(u.x, n); p[1] = norm_u8(u.y, n); p[2] = norm_u8(u.z, n); p[3] = norm_u8(u.w, n);
    } else {
        const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(pred) + i);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}
__device__ __forceinline__ void load_g4(const uint8_t* gt, int64_t i, int gthr, bool* g) {
    const uchar4 u = *reinterpret_cast<const uchar4*>(gt + i);
    g[0] = u.x > gthr; g[1] = u.y > gthr; g[2] = u.z > gthr; g[3] = u.w > gthr;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
