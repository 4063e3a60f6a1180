// Fused global self-attention (keras MultiHeadAttention inside backbones/vit.py:142-147,166 and the sliding-window driver of
// core_inference.py): O = softmax(scale * Q K^T) V for packed qkv [B, T, 3*heads*64] bf16, head_dim 64, any T.  One wavefront owns
// 64 query rows of one (sample, head) and walks the keys in tiles of 64 with the online-softmax recurrence (running row max m and
// row sum l, accumulator rescaled by exp(m_old - m_new)), so the T x T score matrix -- 12 x 1025 x 1025 per ViT-B window, written
// and re-read twice by the GEMM + softmax route -- never exists.  The tile bodies are those of attn_tile.h; this file is the
// (sample, head, tile) item decode on the packed tensor, the row-dot kernel and the launchers.
//
// Training.  The forward kernel also returns L[i] = log2 sum_j exp2(c * s_ij) (c = scale * log2 e); the backward pass recomputes
// the probabilities tile by tile from q, k and L (p = exp2(c * s - L): no running maximum).  With D[i] = sum_d dO[i][d] * O[i][d]:
//     dS = P o (dP - D) * scale,  dP = dO V^T,      dV = P^T dO        dK = dS^T Q        dQ = dS K.
// Two tile kernels, no atomics, fixed summation order (deterministic): flash_attn_dq_kernel (a wavefront owns 64 queries) and
// flash_attn_dkdv_kernel (a wavefront owns 64 keys).
#include "attn_tile.h"
#include "iseg_hip.h"

namespace {

using namespace attn;

// item = (b * heads + h) * tiles + tile: one 64-row tile of one (sample, head) of the packed tensor (row pitch 3C)
struct FlashItem {
    int tile, h;
    int64_t b, bh;
    const bf16_t *q, *k, *v;
};
__device__ __forceinline__ FlashItem flash_item(const bf16_t* __restrict__ qkv, int64_t item, int T, int heads, int tiles) {
    FlashItem it;
    it.tile = (int)(item % tiles);
    it.bh = item / tiles;
    it.h = (int)(it.bh % heads);
    it.b = it.bh / heads;
    const int C = heads * AD;
    const int64_t ld = 3 * C;
    it.q = qkv + it.b * T * ld + it.h * AD;
    it.k = it.q + C;
    it.v = it.q + 2 * C;
    return it;
}

__global__ __launch_bounds__(128) void flash_attn_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                             float* __restrict__ lse2, int64_t items, int T, int heads, int qtiles,
                                                             float scale) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Vl = reinterpret_cast<bf16_t*>(fsm) + (size_t)wv * (AK * ASTRIDE);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const FlashItem it = flash_item(qkv, item, T, heads, qtiles);
    const int C = heads * AD;
    const int64_t ld = 3 * C;
    // keys past T: exp2 underflows to zero from the -FLT_MAX score at every scale this route is given, no explicit zero
    attn_fwd_tile<false>(it.q, ld, it.k, ld, it.v, ld, out + it.b * T * C, C, it.h * AD,
                         lse2 + it.bh * ((int64_t)qtiles * AQ), lse2 != nullptr, it.tile, T, scale, Vl, lane);
}

// D[(b*heads + h) * Tp + i] = sum_d dO[b][i][h*64 + d] * O[b][i][h*64 + d]
__global__ __launch_bounds__(256) void flash_attn_rowdot_kernel(const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                                float* __restrict__ dsum, int64_t B, int T, int heads, int Tp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (b, i, h), h fastest: a wavefront reads contiguous rows
    if (idx >= B * T * heads) return;
    const int h = (int)(idx % heads);
    const int64_t bi = idx / heads;
    const int i = (int)(bi % T);
    const int64_t b = bi / T;
    const bf16_t* o = out + bi * heads * AD + h * AD;
    const bf16_t* d = dout + bi * heads * AD + h * AD;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < AD; k += 8) {
        float a[8], g[8];
        load8<bf16_t>(o + k, a);
        load8<bf16_t>(d + k, g);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_fmaf(a[u], g[u], acc);
    }
    dsum[(b * heads + h) * Tp + i] = acc;
}

__global__ __launch_bounds__(128) void flash_attn_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                            const float* __restrict__ lse2, const float* __restrict__ dsum,
                                                            bf16_t* __restrict__ dqkv, int64_t items, int T, int heads, int qtiles,
                                                            float scale) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Kl = reinterpret_cast<bf16_t*>(fsm) + (size_t)wv * (AK * ASTRIDE);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const int qt = (int)(item % qtiles);
    const int64_t bh = item / qtiles;
    const int h = (int)(bh % heads);
    const int64_t b = bh / heads;
    const int C = heads * AD;
    const int64_t ld = 3 * C;
    const bf16_t* qb = qkv + b * T * ld + h * AD;
    const bf16_t* kb = qb + C;
    const bf16_t* vb = qb + 2 * C;
    const bf16_t* dob = dout + b * T * C + h * AD;
    const int q0 = qt * AQ;
    const int jl = lane & 15, g4 = (lane >> 4) * 4;
    const float c = scale * LOG2E;
    const int vrow = lane >> 3, vcol = (lane & 7) * 8;

    bf16x8 aq[4][2], ado[4][2], vf[4][2], kr[8];
    float L[4], Dd[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            aq[ti][ks] = gfrag(qb, ld, q0 + ti * 16 + jl, T, ks * 32, lane);
            ado[ti][ks] = gfrag(dob, C, q0 + ti * 16 + jl, T, ks * 32, lane);
        }
        const int64_t li = bh * ((int64_t)qtiles * AQ) + q0 + ti * 16 + jl;
        L[ti] = lse2[li];
        Dd[ti] = dsum[li];
    }
    auto fetch = [&](int k0) {
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) vf[tj][ks] = gfrag(vb, ld, k0 + tj * 16 + jl, T, ks * 32, lane);
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            const int row = k0 + vrow + 8 * cc;
            kr[cc] = (row < T) ? *reinterpret_cast<const bf16x8*>(kb + (int64_t)row * ld + vcol) : zero8();
        }
    };
    fetch(0);
    f32x4 dq[4][4];      // [td][ti]: dQ[i = ti*16 + jl][d = td*16 + g4 + r]
#pragma unroll
    for (int td = 0; td < 4; ++td)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) dq[td][ti] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < T; k0 += AK) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) *reinterpret_cast<bf16x8*>(Kl + (vrow + 8 * cc) * ASTRIDE + vcol) = kr[cc];
        __builtin_amdgcn_wave_barrier();
        f32x4 s[4][4], dp[4][4];      // [tj][ti]: key k0 + tj*16 + g4 + r, query q0 + ti*16 + jl
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) s[tj][ti] = dp[tj][ti] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                const bf16x8 kf = row_frag(Kl, ASTRIDE, tj * 16, ks * 32, lane);
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) {
                    s[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, aq[ti][ks], s[tj][ti], 0, 0, 0);
                    dp[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[tj][ks], ado[ti][ks], dp[tj][ti], 0, 0, 0);
                }
            }
        const bool ragged = k0 + AK > T;
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[tj][ti][r], c, -L[ti]));
                    if (ragged && k0 + tj * 16 + g4 + r >= T) p = 0.f;
                    s[tj][ti][r] = p * (dp[tj][ti][r] - Dd[ti]) * scale;
                }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 bds[4], akt[4];
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bds[ti][r] = (bf16_t)s[2 * ks][ti][r];
                    bds[ti][4 + r] = (bf16_t)s[2 * ks + 1][ti][r];
                }
#pragma unroll
            for (int td = 0; td < 4; ++td) akt[td] = ltfrag(Kl, 32 * ks, 32 * ks + 16, td * 16, lane);
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) dq[td][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akt[td], bds[ti], dq[td][ti], 0, 0, 0);
        }
        if (k0 + AK < T) fetch(k0 + AK);
        __builtin_amdgcn_wave_barrier();
    }
    bf16_t* dqb = dqkv + b * T * ld + h * AD;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int i = q0 + ti * 16 + jl;
        if (i < T) {
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16_t)dq[td][ti][r];
                *reinterpret_cast<bf16x4*>(dqb + (int64_t)i * ld + td * 16 + g4) = w;
            }
        }
    }
}

// rows past T hold zero q / dO (their terms vanish), columns past T are never stored: no masking needed
__global__ __launch_bounds__(128) void flash_attn_dkdv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                              const float* __restrict__ lse2, const float* __restrict__ dsum,
                                                              bf16_t* __restrict__ dqkv, int64_t items, int T, int heads, int qtiles,
                                                              float scale) {
    extern __shared__ __attribute__((aligned(16))) char fsm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Ql = reinterpret_cast<bf16_t*>(fsm) + (size_t)wv * (2 * AI * ASTRIDE);
    bf16_t* Ol = Ql + AI * ASTRIDE;
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const FlashItem it = flash_item(qkv, item, T, heads, qtiles);
    const int C = heads * AD;
    const int64_t ld = 3 * C, row = it.bh * ((int64_t)qtiles * AQ);
    bf16_t* dkb = dqkv + it.b * T * ld + C + it.h * AD;
    attn_key_tile<true, true, true, false>(it.q, ld, it.k, ld, it.v, ld, dout + it.b * T * C + it.h * AD, C, lse2 + row, dsum + row, dkb,
                                           ld, dkb + C, ld, it.tile, T, AD, scale, Ql, Ol, lane);
}

}  // namespace

extern "C" int iseg_attention_fwd_supported(int head_dim, int dtype) { return (head_dim == AD && dtype == ISEG_BF16) ? 1 : 0; }

static int launch_attention_fwd(const void* qkv, void* out, float* lse2, int64_t batch, int T, int heads, int head_dim, float scale,
                                int dtype, hipStream_t stream, const char* who) {
    ISEG_REQUIRE(qkv && out && batch > 0 && T > 0 && heads > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(iseg_attention_fwd_supported(head_dim, dtype), "%s: needs bf16 and head_dim 64 (got %d)", who, head_dim);
    ISEG_REQUIRE(((uintptr_t)qkv | (uintptr_t)out) % 16 == 0, "%s: operands must be 16-byte aligned", who);
    const int qtiles = (T + AQ - 1) / AQ;
    const int64_t items = batch * heads * qtiles;
    const size_t lds = (size_t)2 * AK * ASTRIDE * sizeof(bf16_t);
    hipLaunchKernelGGL(flash_attn_fwd_kernel, dim3((unsigned)ceil_div64(items, 2)), dim3(128), lds, stream, (const bf16_t*)qkv,
                       (bf16_t*)out, lse2, items, T, heads, qtiles, scale);
    return iseg_check_launch(who);
}

extern "C" int iseg_attention_fwd(const void* qkv, void* out, int64_t batch, int T, int heads, int head_dim, float scale, int dtype,
                                  hipStream_t stream) {
    return launch_attention_fwd(qkv, out, nullptr, batch, T, heads, head_dim, scale, dtype, stream, "iseg_attention_fwd");
}

extern "C" size_t iseg_attention_lse_elems(int64_t batch, int T, int heads) {
    return (size_t)batch * heads * (size_t)((T + AQ - 1) / AQ * AQ);
}

extern "C" int iseg_attention_fwd_train(const void* qkv, void* out, float* lse2, int64_t batch, int T, int heads, int head_dim,
                                        float scale, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(lse2 && (uintptr_t)lse2 % 16 == 0, "iseg_attention_fwd_train: lse2 must be a 16-byte aligned buffer");
    return launch_attention_fwd(qkv, out, lse2, batch, T, heads, head_dim, scale, dtype, stream, "iseg_attention_fwd_train");
}

extern "C" size_t iseg_attention_bwd_workspace_bytes(int64_t batch, int T, int heads) {
    return iseg_attention_lse_elems(batch, T, heads) * sizeof(float);
}

extern "C" int iseg_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse2, void* dqkv, int64_t batch, int T,
                                  int heads, int head_dim, float scale, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(qkv && out && dout && lse2 && dqkv && batch > 0 && T > 0 && heads > 0, "iseg_attention_bwd: bad arguments");
    ISEG_REQUIRE(iseg_attention_fwd_supported(head_dim, dtype), "iseg_attention_bwd: needs bf16 and head_dim 64 (got %d)", head_dim);
    ISEG_REQUIRE(((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv | (uintptr_t)lse2) % 16 == 0,
                 "iseg_attention_bwd: operands must be 16-byte aligned");
    const size_t need = iseg_attention_bwd_workspace_bytes(batch, T, heads);
    ISEG_NEED_WORKSPACE("iseg_attention_bwd", ws, ws_bytes, need);
    ISEG_REQUIRE_WORKSPACE((uintptr_t)ws % 16 == 0, "iseg_attention_bwd: the workspace must be 16-byte aligned");
    float* dsum = (float*)ws;
    const int qtiles = (T + AQ - 1) / AQ;
    const int Tp = qtiles * AQ;
    const int64_t items = batch * heads * qtiles;
    hipMemsetAsync(dsum, 0, need, stream);      // rows T .. Tp-1 are read (as zeros) by the tile loops
    hipLaunchKernelGGL(flash_attn_rowdot_kernel, dim3((unsigned)ceil_div64(batch * T * heads, 256)), dim3(256), 0, stream,
                       (const bf16_t*)out, (const bf16_t*)dout, dsum, batch, T, heads, Tp);
    hipLaunchKernelGGL(flash_attn_dq_kernel, dim3((unsigned)ceil_div64(items, 2)), dim3(128), (size_t)2 * AK * ASTRIDE * sizeof(bf16_t),
                       stream, (const bf16_t*)qkv, (const bf16_t*)dout, lse2, dsum, (bf16_t*)dqkv, items, T, heads, qtiles, scale);
    hipLaunchKernelGGL(flash_attn_dkdv_kernel, dim3((unsigned)ceil_div64(items, 2)), dim3(128),
                       (size_t)2 * 2 * AI * ASTRIDE * sizeof(bf16_t), stream, (const bf16_t*)qkv, (const bf16_t*)dout, lse2, dsum,
                       (bf16_t*)dqkv, items, T, heads, qtiles, scale);
    return iseg_check_launch("iseg_attention_bwd");
}
