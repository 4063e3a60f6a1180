// Single-head attention core of the non-local block (layers/self_attention.py:65-93 with get_attention of
// utils/attention_utils.py:23-40): O = softmax(scale * Q K^T) V for a 64-wide query / key and a WIDE value (dv = 64 .. 1024 in
// steps of 64), bf16, any T, every operand with its own row pitch (column ranges of one packed projection output or separate
// tensors; q and k may be one pointer).  The tile bodies are those of attn_tile.h, run over value slabs of 64 columns: a forward
// work item is (sample, 64-query tile, value slab) and owns one wavefront with the register budget and LDS image of the
// equal-width kernel; each slab recomputes S^T.  Nothing of size T x T is ever stored.
//
// Training: the forward also returns L[i] = log2 sum_j exp2(c * s_ij) (c = scale * log2 e), written by slab 0; the backward pass
// recomputes p = exp2(c * s - L) tile by tile.  With D[i] = sum over ALL dv columns of dO[i][.] * O[i][.]:
//     dV = P^T dO      dP = dO V^T (contracted over the whole dv)      dS = P o (dP - D) * scale      dQ = dS K      dK = dS^T Q
// Four kernels, no atomics, fixed summation order (a second run is bit-identical):
//   * self_attn_rowdot_kernel -- D, eight lanes per row, combined in a fixed butterfly;
//   * self_attn_dv_kernel     -- (sample, key tile, value slab) walks the query rows 32 at a time: S = Q K^T, dV^T += dO^T P;
//   * self_attn_dq_kernel     -- (sample, query tile) walks the key tiles in the forward's transposed orientation;
//   * self_attn_dk_kernel     -- (sample, key tile) walks the query rows 32 at a time in the natural orientation.
// The dO / V fragments of the full-width dP product are streamed (attn_tile.h).  Any positive finite scale is accepted, so nothing
// here leans on an exp2 underflow: key columns >= T of a ragged last tile get probability exactly 0, and the key-owning kernels
// switch rows and keys past T off explicitly.
#include "attn_tile.h"
#include "iseg_hip.h"

#include <limits.h>

namespace {

using namespace attn;

constexpr int SDV_MAX = 1024;

// item = ((b * qtiles) + qt) * slabs + slab: the slabs of one query tile are neighbours, their K tiles meet in L2
__global__ __launch_bounds__(128) void self_attn_fwd_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                            int64_t ldk, const bf16_t* __restrict__ v, int64_t ldv,
                                                            bf16_t* __restrict__ out, int64_t ldo, float* __restrict__ lse2,
                                                            int64_t items, int T, int qtiles, int slabs, float scale) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Vl = reinterpret_cast<bf16_t*>(ssm) + (size_t)wv * (AK * ASTRIDE);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const int slab = (int)(item % slabs);
    const int64_t bq = item / slabs;
    const int qt = (int)(bq % qtiles);
    const int64_t b = bq / qtiles;
    // every slab of a row computes the same L, slab 0 writes it
    attn_fwd_tile<true>(q + b * T * ldq, ldq, k + b * T * ldk, ldk, v + b * T * ldv + slab * AD, ldv, out + b * T * ldo, ldo, slab * AD,
                        lse2 + b * ((int64_t)qtiles * AQ), lse2 && slab == 0, qt, T, scale, Vl, lane);
}

// D[b * Tp + i] = sum_c dO[b][i][c] * O[b][i][c] over all dv columns: eight lanes per row, lane `sub` takes the 8-column chunks
// sub, sub + 8, ... (dv % 64 == 0: every lane the same count), then a fixed three-step butterfly
__global__ __launch_bounds__(256) void self_attn_rowdot_kernel(const bf16_t* __restrict__ out, int64_t ldo, const bf16_t* __restrict__ dout,
                                                               int64_t lddo, float* __restrict__ dsum, int64_t rows, int T, int Tp, int dv) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx >> 3;
    const int sub = (int)(idx & 7);
    const bool live = row < rows;
    float acc = 0.f;
    int64_t b = 0;
    int i = 0;
    if (live) {
        b = row / T;
        i = (int)(row % T);
        const bf16_t* o = out + (b * T + i) * ldo;
        const bf16_t* d = dout + (b * T + i) * lddo;
        for (int c0 = sub * 8; c0 < dv; c0 += 64) {
            float a[8], g[8];
            load8<bf16_t>(o + c0, a);
            load8<bf16_t>(d + c0, g);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_fmaf(a[u], g[u], acc);
        }
    }
    acc += xorf(acc, 1);
    acc += xorf(acc, 2);
    acc += xorf(acc, 4);
    if (live && sub == 0) dsum[b * Tp + i] = acc;
}

// item = (b * qtiles) + qt
__global__ __launch_bounds__(128) void self_attn_dq_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                           const bf16_t* __restrict__ v, int64_t ldv, const bf16_t* __restrict__ dout,
                                                           int64_t lddo, const float* __restrict__ lse2, const float* __restrict__ dsum,
                                                           bf16_t* __restrict__ dq_out, int64_t lddq, int64_t items, int T, int qtiles, int dv,
                                                           float scale) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Kl = reinterpret_cast<bf16_t*>(ssm) + (size_t)wv * (AK * ASTRIDE);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const int qt = (int)(item % qtiles);
    const int64_t b = item / qtiles;
    const bf16_t* qb = q + b * T * ldq;
    const bf16_t* kb = k + b * T * ldk;
    const bf16_t* vb = v + b * T * ldv;
    const bf16_t* dob = dout + b * T * lddo;
    const int q0 = qt * AQ;
    const int jl = lane & 15, g4 = (lane >> 4) * 4;
    const float c = scale * LOG2E;
    const int vrow = lane >> 3, vcol = (lane & 7) * 8;

    bf16x8 aq[4][2], kr[8];
    float L[4], Dd[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) aq[ti][ks] = gfrag(qb, ldq, q0 + ti * 16 + jl, T, ks * 32, lane);
        const int64_t li = b * ((int64_t)qtiles * AQ) + q0 + ti * 16 + jl;
        L[ti] = lse2[li];
        Dd[ti] = dsum[li];
    }
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) kr[cc] = grow8(kb, ldk, vrow + 8 * cc, T, vcol);
    f32x4 dq[4][4];      // [td][ti]: dQ[i = ti*16 + jl][d = td*16 + g4 + r]
#pragma unroll
    for (int td = 0; td < 4; ++td)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) dq[td][ti] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < T; k0 += AK) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) *reinterpret_cast<bf16x8*>(Kl + (vrow + 8 * cc) * ASTRIDE + vcol) = kr[cc];
        __builtin_amdgcn_wave_barrier();
        if (k0 + AK < T) {      // next K tile flies during this tile's products
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) kr[cc] = grow8(kb, ldk, k0 + AK + vrow + 8 * cc, T, vcol);
        }
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
                for (int ti = 0; ti < 4; ++ti) s[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, aq[ti][ks], s[tj][ti], 0, 0, 0);
            }
        // dP^T = V dO^T over the whole value width, 32 columns per step
#pragma unroll 2
        for (int c0 = 0; c0 < dv; c0 += 32) {
            bf16x8 vf[4], ad[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                vf[t] = gfrag(vb, ldv, k0 + t * 16 + jl, T, c0, lane);
                ad[t] = gfrag(dob, lddo, q0 + t * 16 + jl, T, c0, lane);
            }
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) dp[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[tj], ad[ti], dp[tj][ti], 0, 0, 0);
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
        __builtin_amdgcn_wave_barrier();
    }
    bf16_t* dqb = dq_out + b * T * lddq;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int i = q0 + ti * 16 + jl;
        if (i < T) {
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16_t)dq[td][ti][r];
                *reinterpret_cast<bf16x4*>(dqb + (int64_t)i * lddq + td * 16 + g4) = w;
            }
        }
    }
}

// item = (b * ktiles) + kt
__global__ __launch_bounds__(128) void self_attn_dk_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                           const bf16_t* __restrict__ v, int64_t ldv, const bf16_t* __restrict__ dout,
                                                           int64_t lddo, const float* __restrict__ lse2, const float* __restrict__ dsum,
                                                           bf16_t* __restrict__ dk_out, int64_t lddk, int64_t items, int T, int ktiles, int dv,
                                                           float scale) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Ql = reinterpret_cast<bf16_t*>(ssm) + (size_t)wv * (AI * ASTRIDE);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const int kt = (int)(item % ktiles);
    const int64_t b = item / ktiles, row = b * ((int64_t)ktiles * AQ);
    attn_key_tile<true, false, false, true>(q + b * T * ldq, ldq, k + b * T * ldk, ldk, v + b * T * ldv, ldv, dout + b * T * lddo, lddo,
                                            lse2 + row, dsum + row, dk_out + b * T * lddk, lddk, nullptr, 0, kt, T, dv, scale, Ql, nullptr,
                                            lane);
}

// item = ((b * ktiles) + kt) * slabs + slab; Q is fed as global fragments, the LDS image holds the slab's dO rows
__global__ __launch_bounds__(128) void self_attn_dv_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                           const bf16_t* __restrict__ dout, int64_t lddo, const float* __restrict__ lse2,
                                                           bf16_t* __restrict__ dv_out, int64_t lddv, int64_t items, int T, int ktiles,
                                                           int slabs, float scale) {
    extern __shared__ __attribute__((aligned(16))) char ssm[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bf16_t* Ol = reinterpret_cast<bf16_t*>(ssm) + (size_t)wv * (AI * ASTRIDE);
    const int64_t item = (int64_t)blockIdx.x * 2 + wv;
    if (item >= items) return;
    const int slab = (int)(item % slabs);
    const int64_t bk = item / slabs;
    const int kt = (int)(bk % ktiles);
    const int64_t b = bk / ktiles;
    attn_key_tile<false, true, false, true>(q + b * T * ldq, ldq, k + b * T * ldk, ldk, nullptr, 0, dout + b * T * lddo + slab * AD, lddo,
                                            lse2 + b * ((int64_t)ktiles * AQ), nullptr, nullptr, 0, dv_out + b * T * lddv + slab * AD, lddv,
                                            kt, T, AD, scale, nullptr, Ol, lane);
}

bool pitch_ok(int64_t ld, int width) { return ld >= width && ld % 8 == 0; }

}  // namespace

extern "C" int iseg_self_attention_supported(int dk, int dv, int dtype) {
    return (dtype == ISEG_BF16 && dk == AD && dv >= AD && dv <= SDV_MAX && dv % AD == 0) ? 1 : 0;
}

extern "C" size_t iseg_self_attention_lse_elems(int64_t batch, int T) {
    if (batch <= 0 || T <= 0) return 0;
    return (size_t)batch * (size_t)(((int64_t)T + AQ - 1) / AQ * AQ);
}

#define SELFATTN_UNSUPPORTED(cond, ...)       \
    do {                                      \
        if (!(cond)) {                        \
            iseg_set_error(__VA_ARGS__);      \
            return ISEG_ERR_UNSUPPORTED;      \
        }                                     \
    } while (0)

// the checks both entry points make after their own argument test and before their pitch test
static int self_attn_shape_ok(const char* who, int dk, int dv, float scale, int dtype) {
    SELFATTN_UNSUPPORTED(iseg_self_attention_supported(dk, dv, dtype), "%s: needs bf16, dk 64 and dv a multiple of 64 in 64..1024 (got dk %d, dv %d)",
                         who, dk, dv);
    SELFATTN_UNSUPPORTED(scale > 0.f && scale <= FLT_MAX, "%s: needs a positive finite scale", who);
    return ISEG_OK;
}

extern "C" int iseg_self_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out,
                                       int64_t ldo, float* lse2, int64_t batch, int T, int dk, int dv, float scale, int dtype,
                                       hipStream_t stream) {
    const char* who = "iseg_self_attention_fwd";
    ISEG_REQUIRE(q && k && v && out && batch > 0 && T > 0 && T <= INT_MAX - AQ, "%s: bad arguments", who);
    if (const int rc = self_attn_shape_ok(who, dk, dv, scale, dtype)) return rc;
    SELFATTN_UNSUPPORTED(pitch_ok(ldq, dk) && pitch_ok(ldk, dk) && pitch_ok(ldv, dv) && pitch_ok(ldo, dv),
                         "%s: row pitches must be multiples of 8 elements and cover their rows (got %lld %lld %lld %lld)", who, (long long)ldq,
                         (long long)ldk, (long long)ldv, (long long)ldo);
    SELFATTN_UNSUPPORTED(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)lse2) % 16 == 0,
                         "%s: operands must be 16-byte aligned", who);
    const int qtiles = (T + AQ - 1) / AQ, slabs = dv / AD;
    const int64_t items = batch * qtiles * slabs;
    ISEG_REQUIRE(ceil_div64(items, 2) <= INT_MAX, "%s: too many work items", who);
    hipLaunchKernelGGL(self_attn_fwd_kernel, dim3((unsigned)ceil_div64(items, 2)), dim3(128), (size_t)2 * AK * ASTRIDE * sizeof(bf16_t), stream,
                       (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv, (bf16_t*)out, ldo, lse2, items, T, qtiles, slabs,
                       scale);
    return iseg_check_launch(who);
}

extern "C" int iseg_self_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* out,
                                       int64_t ldo, const void* dout, int64_t lddo, const float* lse2, float* dsum, void* dq, int64_t lddq,
                                       void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t batch, int T, int dk_dim, int dv_dim,
                                       float scale, int dtype, hipStream_t stream) {
    const char* who = "iseg_self_attention_bwd";
    ISEG_REQUIRE(q && k && v && out && dout && lse2 && dsum && dq && dk && dv && batch > 0 && T > 0 && T <= INT_MAX - AQ, "%s: bad arguments",
                 who);
    if (const int rc = self_attn_shape_ok(who, dk_dim, dv_dim, scale, dtype)) return rc;
    SELFATTN_UNSUPPORTED(pitch_ok(ldq, dk_dim) && pitch_ok(ldk, dk_dim) && pitch_ok(ldv, dv_dim) && pitch_ok(ldo, dv_dim) &&
                             pitch_ok(lddo, dv_dim) && pitch_ok(lddq, dk_dim) && pitch_ok(lddk, dk_dim) && pitch_ok(lddv, dv_dim),
                         "%s: row pitches must be multiples of 8 elements and cover their rows", who);
    SELFATTN_UNSUPPORTED(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)lse2 | (uintptr_t)dsum |
                          (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % 16 == 0,
                         "%s: operands must be 16-byte aligned", who);
    ISEG_REQUIRE(dq != dk, "%s: dq and dk must be separate buffers (the caller adds them when q and k alias)", who);
    const int tiles = (T + AQ - 1) / AQ, slabs = dv_dim / AD;
    const int Tp = tiles * AQ;
    const int64_t items = batch * tiles, rows = batch * T;
    ISEG_REQUIRE(ceil_div64(items * slabs, 2) <= INT_MAX && ceil_div64(rows * 8, 256) <= INT_MAX, "%s: too many work items", who);
    const bf16_t *qp = (const bf16_t*)q, *kp = (const bf16_t*)k, *vp = (const bf16_t*)v, *dop = (const bf16_t*)dout;
    hipMemsetAsync(dsum, 0, iseg_self_attention_lse_elems(batch, T) * sizeof(float), stream);      // rows T .. Tp-1 are read by the tile loops
    hipLaunchKernelGGL(self_attn_rowdot_kernel, dim3((unsigned)ceil_div64(rows * 8, 256)), dim3(256), 0, stream, (const bf16_t*)out, ldo, dop,
                       lddo, dsum, rows, T, Tp, dv_dim);
    hipLaunchKernelGGL(self_attn_dv_kernel, dim3((unsigned)ceil_div64(items * slabs, 2)), dim3(128), (size_t)2 * AI * ASTRIDE * sizeof(bf16_t),
                       stream, qp, ldq, kp, ldk, dop, lddo, lse2, (bf16_t*)dv, lddv, items * slabs, T, tiles, slabs, scale);
    hipLaunchKernelGGL(self_attn_dq_kernel, dim3((unsigned)ceil_div64(items, 2)), dim3(128), (size_t)2 * AK * ASTRIDE * sizeof(bf16_t), stream,
                       qp, ldq, kp, ldk, vp, ldv, dop, lddo, lse2, dsum, (bf16_t*)dq, lddq, items, T, tiles, dv_dim, scale);
    hipLaunchKernelGGL(self_attn_dk_kernel, dim3((unsigned)ceil_div64(items, 2)), dim3(128), (size_t)2 * AI * ASTRIDE * sizeof(bf16_t), stream,
                       qp, ldq, kp, ldk, vp, ldv, dop, lddo, lse2, dsum, (bf16_t*)dk, lddk, items, T, tiles, dv_dim, scale);
    return iseg_check_launch(who);
}
