// Shared by the weight-gradient kernels of the fused ConvNeXt MLP (mlp_wgrad.hip, mlp_bwd_onepass.hip): the 16x16x32 MFMA wrapper, the
// transposed B fragment of a row-major LDS tile, the layout of the chunk-record workspace, and the tail both launchers end on: records -> their
// sum -> the finish launch that books the parameter gradients from the chunk-summed record -> the layer-scale gradient's second stage.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// B fragment (lane = channel 16 cb + (lane & 15)) of the 32 tile rows at `rows` in the accumulator's row order: k slot (q, j) = row 4 q + j
// (j < 4), 16 + 4 q + j - 4 (j >= 4)
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* rows, int stride, int cb, int lane) {
    const int q = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3;
    const bf16_t* a0 = rows + (4 * q + qq) * stride + 16 * cb + 4 * p;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(a0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(a0 + 16 * stride));
    bf16x8 f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[i] = lo[i];
        f[4 + i] = hi[i];
    }
    return f;
}

// Book the parameter gradients from the chunk-summed record (accumulating into the flat gradient buffer):
//     dW1[c][hid] += dW1T[hid][c]      db1[hid] += ..      dW2[hid][c] += Z[hid][c] gamma[c]      db2[c] += gamma[c] S[c]
//     dgamma[c]   += sum_hid W2[hid][c] Z[hid][c] + b2[c] S[c]           (gamma == NULL: dW2 += Z, db2 += S)
// Block = 8 hidden units x 32 channels (256 threads, one element each); dW1 leaves through an LDS transpose; the per-block column sums of
// W2 o Z go to `gpart` [HID / 8][C] for the fixed-order second stage.  (Summing the 80 chunk records inside this kernel took 47-134 us in
// three different shapes -- 144 workgroups cannot pull 24 MB, and the db1 / S sums were 80 dependent loads on a handful of threads; the
// generic row reduction in front does it in 8.5 us.)
constexpr int FIN_ROWS = 8;
// `rec` = the chunk-summed record [Z | dW1T | db1 | S] (fp32, one fixed-order row reduction over the chunk records in front of this launch)
__global__ __launch_bounds__(256) void convnext_mlp_wgrad_finish_kernel(const float* __restrict__ rec, const float* __restrict__ W2,
                                                                        const float* __restrict__ b2, const float* __restrict__ gamma,
                                                                        float* __restrict__ dW1, float* __restrict__ db1,
                                                                        float* __restrict__ dW2, float* __restrict__ db2,
                                                                        float* __restrict__ gpart, int C) {
    __shared__ float tw[FIN_ROWS][33];
    __shared__ float tg[8][32];
    const int HID = 4 * C;
    const int c0 = blockIdx.x * 32, h0 = blockIdx.y * FIN_ROWS;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const int c = c0 + tx;
    const int64_t plane = (int64_t)HID * C;
    const float gm = gamma ? gamma[c] : 1.f;
    {
        const int64_t o = (int64_t)(h0 + ty) * C + c;
        const float z = rec[o], w = rec[plane + o];
        dW2[o] += z * gm;
        tg[ty][tx] = W2[o] * z;
        tw[ty][tx] = w;
    }
    __syncthreads();
    {      // dW1[c][hid]: thread -> (channel row, hidden unit): FIN_ROWS consecutive hidden units per channel
        const int hx = threadIdx.x & (FIN_ROWS - 1), cc = threadIdx.x / FIN_ROWS;      // 8 x 32
        dW1[(int64_t)(c0 + cc) * HID + h0 + hx] += tw[hx][cc];
    }
    if (ty == 0) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v += tg[j][tx];
        if (blockIdx.y == 0) {
            const float s = rec[2 * plane + HID + c];
            if (gamma) {
                v += b2[c] * s;
                db2[c] += gm * s;
            } else {
                db2[c] += s;
            }
        }
        if (gamma) gpart[(int64_t)blockIdx.y * C + c] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < FIN_ROWS) {
        const int hid = h0 + threadIdx.x;
        db1[hid] += rec[2 * plane + hid];
    }
}

// floats of one chunk record [Z | dW1T | db1 | S]: what a producer workgroup leaves per row chunk, and what the finish kernel reads summed
constexpr int64_t mlp_record_floats(int C) {
    const int64_t HID = 4 * C;
    return 2 * HID * C + HID + C;
}

// The producers' workspace: [records | sum | layer-scale partials | LayerNorm partial rows] (the last for the one-pass kernel only)
struct MlpGradWs {
    int C, nchunk;
    bool with_ln;
    int64_t rec() const { return mlp_record_floats(C); }
    int gparts() const { return 4 * C / FIN_ROWS; }      // rows the finish launch leaves for the layer-scale gradient
    float* records(float* ws) const { return ws; }
    float* sum(float* ws) const { return ws + nchunk * rec(); }
    float* gpart(float* ws) const { return sum(ws) + rec(); }
    float* lnpart(float* ws) const { return gpart(ws) + (int64_t)gparts() * C; }
    size_t floats() const { return (size_t)((nchunk + 1) * rec() + (int64_t)gparts() * C + (with_ln ? (int64_t)nchunk * 2 * C : 0)); }
};

// The tail of both producers: chunk records -> their sum (the fixed-order row reduction of common.h) -> the finish launch -> dgamma, queued
// when the caller defers reductions.  `who` names the entry point in a launch error.
inline int mlp_grads_from_records(const MlpGradWs& L, float* ws, const float* W2, const float* b2, const float* gamma, float* dW1, float* db1,
                                  float* dW2, float* db2, float* dgamma, const char* who, hipStream_t stream) {
    const int C = L.C, HID = 4 * C;
    launch_reduce_rows({.partials = L.records(ws), .P = L.nchunk, .pstride = L.rec(), .n = L.rec(), .out0 = L.sum(ws), .n0 = L.rec()}, stream);
    RowReduce red{.P = L.gparts(), .pstride = C, .n = C, .out0 = dgamma, .n0 = C, .accumulate = 1};
    float* const gpart = reduce_rows_begin(red, L.gpart(ws), stream, gamma != nullptr);
    hipLaunchKernelGGL(convnext_mlp_wgrad_finish_kernel, dim3(C / 32, HID / FIN_ROWS), dim3(256), 0, stream, L.sum(ws), W2, b2, gamma, dW1, db1, dW2,
                       db2, gpart, C);
    if (gamma) reduce_rows_end(red, stream);
    return iseg_check_launch(who);
}

// Row chunks of the one-pass kernel (mlp_bwd_onepass.hip, C = 96).  It leaves the same chunk records as convnext_mlp_wgrad_kernel, only more
// of them, so ONE size function answers for both launchers at C = 96 (iseg_convnext_mlp_wgrad_workspace_bytes: the larger need).
// One workgroup per CU in ONE resident round (the rule of mlp_wgrad.hip with one hidden group): 256 chunks of whole 64-row tiles.
inline int onepass_rows_per_chunk(int64_t M, int* nchunk) {
    int64_t rpc = (M + 255) / 256;
    rpc = (rpc + 63) / 64 * 64;
    if (rpc < 256) rpc = 256;
    *nchunk = (int)((M + rpc - 1) / rpc);
    return (int)rpc;
}

inline MlpGradWs onepass_ws(int64_t M) {
    int nchunk;
    onepass_rows_per_chunk(M, &nchunk);
    return {96, nchunk, true};
}

}  // namespace
