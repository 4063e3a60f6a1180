// Gemma text backbone (nlp/gemma/*): rotary embedding, causal grouped-query attention with a key-side padding mask, embedding gradient.
//
// Attention (nlp/gemma/gemma_attention.py:116-151, gemma_decoder_block.py:114-136).  The g = nq / nkv query heads that share one key/value
// head are stacked as g * T query rows of ONE problem, stacked row R = t * g + j (token t, head j of the group): a K / V tile is read
// once per group, and the key side sums dK / dV over the group in stacked-row order with no second pass.  The bodies are built from the
// fragment helpers of attn_tile.h (v_mfma_f32_16x16x32_bf16, a wavefront per work item, wave-private LDS images), generalised in three ways:
//   * the query/key contraction runs over h / 32 MFMA k-steps, its fragments streamed from global memory (L1 / L2 hits after the first slab);
//   * the value width is walked in slabs of 64 columns, as selfattn.hip does: a work item owns 64 output columns and recomputes the scores,
//     which keeps every kernel at the register budget of the 64-wide bodies whatever h is (DESIGN.md has the counts);
//   * visibility is explicit: key s is visible to stacked row R iff s <= R / g, s < T and padding_mask[b, s] != 0.  Key tiles wholly above
//     the diagonal of a work item are skipped, every other tile is masked per element.  A masked score never enters the row maximum and its
//     probability is the constant 0, not an exp2 result; while a row has seen no visible key its maximum stays at the sentinel -FLT_MAX,
//     the rescale factor is the constant 0 and no exp2 of a difference of sentinels is formed.  Such rows end with l = 0: out = 0, lse2 = 0,
//     and since the backward kernels apply the same visibility test, dq = 0 and nothing reaches dk / dv.
// Training: L[R] = log2 sum_s exp2(c * s_Rs) (c = scale * log2 e) per stacked row, padded to a multiple of 64 rows per (sample, kv head);
// D[R] = sum_c dO[R][c] O[R][c].  dV = P^T dO, dP = dO V^T, dS = P o (dP - D) * scale, dQ = dS K, dK = dS^T Q.  Four kernels, no atomics,
// fixed summation order: a second run is bit-identical.
#include "attn_tile.h"
#include "iseg_hip.h"

#include <limits.h>

namespace {

using namespace attn;

constexpr int GH_MAX = 256;

// element offset of stacked row R inside one (sample, kv head) problem whose token rows have pitch ld: token R / g, head R % g of the group
__device__ __forceinline__ int64_t stacked_off(int R, int GT, int g, int h, int64_t ld) {
    if (R >= GT) return -1;
    const int t = R / g;
    return (int64_t)t * ld + (int64_t)(R - t * g) * h;
}
__device__ __forceinline__ bf16x8 ofrag(const bf16_t* __restrict__ base, int64_t off, int col) {
    if (off < 0) return zero8();
    return *reinterpret_cast<const bf16x8*>(base + off + col);
}
// visibility bits of the 16 keys k0 + tj * 16 + g4 + r this lane owns in the transposed orientation: bit tj * 4 + r
__device__ __forceinline__ unsigned key_bits(const uint8_t* __restrict__ mrow, int k0, int g4, int T) {
    unsigned bits = 0;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + tj * 16 + g4 + r;
            if (key < T && (!mrow || mrow[key] != 0)) bits |= 1u << (tj * 4 + r);
        }
    return bits;
}

// item = (((b * nkv) + kvh) * qtiles + qt) * slabs + slab: 64 stacked query rows, 64 output columns
__global__ __launch_bounds__(64) void gemma_attn_fwd_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                            const bf16_t* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ mask,
                                                            bf16_t* __restrict__ out, int64_t ldo, float* __restrict__ lse2, int T, int nkv,
                                                            int g, int h, int qtiles, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t Vl[AK * ASTRIDE];
    const int lane = threadIdx.x;
    const int slabs = h / AD;
    int64_t item = blockIdx.x;
    const int slab = (int)(item % slabs);
    item /= slabs;
    const int qt = (int)(item % qtiles);
    item /= qtiles;
    const int kvh = (int)(item % nkv);
    const int64_t b = item / nkv;
    const int GT = g * T, q0 = qt * AQ;
    const int jl = lane & 15, g4 = (lane >> 4) * 4, c8 = 8 * (lane >> 4);
    const float c = scale * LOG2E;
    const int vrow = lane >> 3, vcol = (lane & 7) * 8;

    const bf16_t* qb = q + b * T * ldq + (int64_t)kvh * g * h;
    const bf16_t* kb = k + b * T * ldk + (int64_t)kvh * h;
    const bf16_t* vb = v + b * T * ldv + (int64_t)kvh * h + slab * AD;
    bf16_t* ob = out + b * T * ldo + (int64_t)kvh * g * h + slab * AD;
    const uint8_t* mrow = mask ? mask + b * T : nullptr;

    int64_t qoff[4];
    int tq[4];      // token of the lane's query column per 16-wide tile; -1 past the last row: sees nothing
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int R = q0 + ti * 16 + jl;
        qoff[ti] = stacked_off(R, GT, g, h, ldq);
        tq[ti] = R < GT ? R / g : -1;
    }
    const int Rlast = q0 + AQ - 1 < GT ? q0 + AQ - 1 : GT - 1;
    const int tmax = Rlast / g;      // the last token of this tile: key tiles beyond it lie wholly above the diagonal

    f32x4 o[4][4];      // [td][ti]
    float m[4], l[4];
    zero_tiles(o);
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        m[ti] = -FLT_MAX;
        l[ti] = 0.f;
    }

    for (int k0 = 0; k0 <= tmax; k0 += AK) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)
            *reinterpret_cast<bf16x8*>(Vl + (vrow + 8 * cc) * ASTRIDE + vcol) = grow8(vb, ldv, k0 + vrow + 8 * cc, T, vcol);
        const unsigned bits = key_bits(mrow, k0, g4, T);
        f32x4 s[4][4];      // [tj][ti]: key k0 + tj*16 + g4 + r, query q0 + ti*16 + jl
        zero_tiles(s);
        for (int c0 = 0; c0 < h; c0 += 32) {
            bf16x8 kf[4], aq[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                kf[t] = gfrag(kb, ldk, k0 + t * 16 + jl, T, c0, lane);
                aq[t] = ofrag(qb, qoff[t], c0 + c8);
            }
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) s[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[tj], aq[ti], s[tj][ti], 0, 0, 0);
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
            float mx = -FLT_MAX;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool vis = ((bits >> (tj * 4 + r)) & 1u) && k0 + tj * 16 + g4 + r <= tq[ti];
                    if (vis) mx = fmaxf(mx, s[tj][ti][r]);
                }
            mx = fmaxf(mx, xorf(mx, 16));
            mx = fmaxf(mx, xorf(mx, 32));
            const float mnew = fmaxf(m[ti], mx);
            // nothing visible so far (sentinel): no exp2 of a sentinel difference; l and o are still zero
            const float alpha = m[ti] == -FLT_MAX ? 0.f : __builtin_amdgcn_exp2f((m[ti] - mnew) * c);
            const float mc = mnew == -FLT_MAX ? 0.f : mnew * c;
            m[ti] = mnew;
            float sum = 0.f;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool vis = ((bits >> (tj * 4 + r)) & 1u) && k0 + tj * 16 + g4 + r <= tq[ti];
                    const float pv = vis ? recompute_p(s[tj][ti][r], c, mc) : 0.f;
                    s[tj][ti][r] = pv;
                    sum += pv;
                }
            l[ti] = l[ti] * alpha + sum;
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[td][ti][r] *= alpha;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 bp[4], av[4];
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) bp[ti] = pack_b(s[2 * ks][ti], s[2 * ks + 1][ti]);
#pragma unroll
            for (int td = 0; td < 4; ++td) av[td] = ltfrag(Vl, 32 * ks, 32 * ks + 16, td * 16, lane);
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) o[td][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[td], bp[ti], o[td][ti], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    const int Tp = qtiles * AQ;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        float lt = l[ti];
        lt += xorf(lt, 16);
        lt += xorf(lt, 32);
        const bool any = lt > 0.f;
        const float inv = any ? __frcp_rn(lt) : 0.f;
        const int R = q0 + ti * 16 + jl;
        if (lse2 && slab == 0 && g4 == 0) lse2[(b * nkv + kvh) * (int64_t)Tp + R] = (R < GT && any) ? __builtin_fmaf(m[ti], c, __log2f(lt)) : 0.f;
        if (R < GT) {
            const int t = R / g;
            bf16_t* orow = ob + (int64_t)t * ldo + (int64_t)(R - t * g) * h;
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16_t)(o[td][ti][r] * inv);
                *reinterpret_cast<bf16x4*>(orow + td * 16 + g4) = w;
            }
        }
    }
}

// D[(b * nkv + kvh) * Tp + t * g + j] = sum_c dO[b][t][n][c] * O[b][t][n][c], n = kvh * g + j: eight lanes per (token, head), fixed butterfly
__global__ __launch_bounds__(256) void gemma_attn_rowdot_kernel(const bf16_t* __restrict__ out, int64_t ldo, const bf16_t* __restrict__ dout,
                                                                int64_t lddo, float* __restrict__ dsum, int64_t rows, int T, int nq, int g,
                                                                int h, int Tp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = idx >> 3;
    const int sub = (int)(idx & 7);
    const bool live = row < rows;
    float acc = 0.f;
    int64_t dst = 0;
    if (live) {
        const int n = (int)(row % nq);
        const int64_t bt = row / nq;
        const int t = (int)(bt % T);
        const int64_t b = bt / T;
        const int kvh = n / g, j = n - kvh * g, nkv = nq / g;
        dst = (b * nkv + kvh) * (int64_t)Tp + (int64_t)t * g + j;
        const bf16_t* o = out + bt * ldo + (int64_t)n * h;
        const bf16_t* d = dout + bt * lddo + (int64_t)n * h;
        for (int c0 = sub * 8; c0 < h; c0 += 64) {
            float a[8], gg[8];
            load8<bf16_t>(o + c0, a);
            load8<bf16_t>(d + c0, gg);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_fmaf(a[u], gg[u], acc);
        }
    }
    acc += xorf(acc, 1);
    acc += xorf(acc, 2);
    acc += xorf(acc, 4);
    if (live && sub == 0) dsum[dst] = acc;
}

// item as in the forward: 64 stacked query rows, 64 columns of dQ; walks the visible key tiles in the forward's transposed orientation
__global__ __launch_bounds__(64) void gemma_attn_dq_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                           const bf16_t* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ mask,
                                                           const bf16_t* __restrict__ dout, int64_t lddo, const float* __restrict__ lse2,
                                                           const float* __restrict__ dsum, bf16_t* __restrict__ dq_out, int64_t lddq, int T,
                                                           int nkv, int g, int h, int qtiles, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t Kl[AK * ASTRIDE];
    const int lane = threadIdx.x;
    const int slabs = h / AD;
    int64_t item = blockIdx.x;
    const int slab = (int)(item % slabs);
    item /= slabs;
    const int qt = (int)(item % qtiles);
    item /= qtiles;
    const int kvh = (int)(item % nkv);
    const int64_t b = item / nkv;
    const int GT = g * T, q0 = qt * AQ;
    const int jl = lane & 15, g4 = (lane >> 4) * 4, c8 = 8 * (lane >> 4);
    const float c = scale * LOG2E;
    const int vrow = lane >> 3, vcol = (lane & 7) * 8;

    const bf16_t* qb = q + b * T * ldq + (int64_t)kvh * g * h;
    const bf16_t* dob = dout + b * T * lddo + (int64_t)kvh * g * h;
    const bf16_t* kb = k + b * T * ldk + (int64_t)kvh * h;
    const bf16_t* vb = v + b * T * ldv + (int64_t)kvh * h;
    bf16_t* dqb = dq_out + b * T * lddq + (int64_t)kvh * g * h + slab * AD;
    const uint8_t* mrow = mask ? mask + b * T : nullptr;
    const int64_t lrow = (b * nkv + kvh) * ((int64_t)qtiles * AQ);

    int64_t qoff[4], dooff[4];
    int tq[4];
    float L[4], Dd[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int R = q0 + ti * 16 + jl;
        qoff[ti] = stacked_off(R, GT, g, h, ldq);
        dooff[ti] = stacked_off(R, GT, g, h, lddo);
        tq[ti] = R < GT ? R / g : -1;
        L[ti] = lse2[lrow + R];
        Dd[ti] = dsum[lrow + R];
    }
    const int Rlast = q0 + AQ - 1 < GT ? q0 + AQ - 1 : GT - 1;
    const int tmax = Rlast / g;
    f32x4 dq[4][4];      // [td][ti]
    zero_tiles(dq);

    for (int k0 = 0; k0 <= tmax; k0 += AK) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)
            *reinterpret_cast<bf16x8*>(Kl + (vrow + 8 * cc) * ASTRIDE + vcol) = grow8(kb + slab * AD, ldk, k0 + vrow + 8 * cc, T, vcol);
        const unsigned bits = key_bits(mrow, k0, g4, T);
        f32x4 s[4][4], dp[4][4];      // [tj][ti]
        zero_tiles(s);
        zero_tiles(dp);
        for (int c0 = 0; c0 < h; c0 += 32) {
            bf16x8 kf[4], aq[4], vf[4], ad[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                kf[t] = gfrag(kb, ldk, k0 + t * 16 + jl, T, c0, lane);
                vf[t] = gfrag(vb, ldv, k0 + t * 16 + jl, T, c0, lane);
                aq[t] = ofrag(qb, qoff[t], c0 + c8);
                ad[t] = ofrag(dob, dooff[t], c0 + c8);
            }
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) {
                    s[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[tj], aq[ti], s[tj][ti], 0, 0, 0);
                    dp[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[tj], ad[ti], dp[tj][ti], 0, 0, 0);
                }
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool vis = ((bits >> (tj * 4 + r)) & 1u) && k0 + tj * 16 + g4 + r <= tq[ti];
                    const float p = recompute_p(s[tj][ti][r], c, L[ti]);
                    s[tj][ti][r] = vis ? p * (dp[tj][ti][r] - Dd[ti]) * scale : 0.f;
                }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 bds[4], akt[4];
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) bds[ti] = pack_b(s[2 * ks][ti], s[2 * ks + 1][ti]);
#pragma unroll
            for (int td = 0; td < 4; ++td) akt[td] = ltfrag(Kl, 32 * ks, 32 * ks + 16, td * 16, lane);
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) dq[td][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(akt[td], bds[ti], dq[td][ti], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int R = q0 + ti * 16 + jl;
        if (R < GT) {
            const int t = R / g;
            bf16_t* row = dqb + (int64_t)t * lddq + (int64_t)(R - t * g) * h;
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16_t)dq[td][ti][r];
                *reinterpret_cast<bf16x4*>(row + td * 16 + g4) = w;
            }
        }
    }
}

// item = (((b * nkv) + kvh) * ktiles + kt) * slabs + slab: 64 keys, 64 columns of dK and of dV; walks the stacked query rows from the
// diagonal on, AI = 32 at a time, in the natural orientation (queries on MFMA rows): the group's heads are summed in stacked-row order
__global__ __launch_bounds__(64) void gemma_attn_dkv_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k, int64_t ldk,
                                                            const bf16_t* __restrict__ v, int64_t ldv, const uint8_t* __restrict__ mask,
                                                            const bf16_t* __restrict__ dout, int64_t lddo, const float* __restrict__ lse2,
                                                            const float* __restrict__ dsum, bf16_t* __restrict__ dk_out, int64_t lddk,
                                                            bf16_t* __restrict__ dv_out, int64_t lddv, int T, int nkv, int g, int h, int ktiles,
                                                            int Tp, float scale) {
    __shared__ __attribute__((aligned(16))) bf16_t Ql[AI * ASTRIDE];
    __shared__ __attribute__((aligned(16))) bf16_t Ol[AI * ASTRIDE];
    const int lane = threadIdx.x;
    const int slabs = h / AD;
    int64_t item = blockIdx.x;
    const int slab = (int)(item % slabs);
    item /= slabs;
    const int kt = (int)(item % ktiles);
    item /= ktiles;
    const int kvh = (int)(item % nkv);
    const int64_t b = item / nkv;
    const int GT = g * T, j0 = kt * AK;
    const int jl = lane & 15, g4 = (lane >> 4) * 4, c8 = 8 * (lane >> 4);
    const float c = scale * LOG2E;

    const bf16_t* qb = q + b * T * ldq + (int64_t)kvh * g * h;
    const bf16_t* dob = dout + b * T * lddo + (int64_t)kvh * g * h;
    const bf16_t* kb = k + b * T * ldk + (int64_t)kvh * h;
    const bf16_t* vb = v + b * T * ldv + (int64_t)kvh * h;
    const float* Lb = lse2 + (b * nkv + kvh) * (int64_t)Tp;
    const float* Db = dsum + (b * nkv + kvh) * (int64_t)Tp;

    bool kvis[4];      // key j0 + tj*16 + jl
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const int key = j0 + tj * 16 + jl;
        kvis[tj] = key < T && (!mask || mask[b * T + key] != 0);
    }
    f32x4 dk[4][4], dvv[4][4];      // [td][tj]: key j0 + tj*16 + jl, column slab*64 + td*16 + g4 + r
    zero_tiles(dk);
    zero_tiles(dvv);

    // the first stacked row that can see key j0 is j0 * g; steps start on multiples of AI
    for (int i0 = (int)(((int64_t)j0 * g) / AI * AI); i0 < GT; i0 += AI) {
        bf16x8 qr[4], dor[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int R = i0 + (lane >> 3) + 8 * cc, col = slab * AD + (lane & 7) * 8;
            qr[cc] = ofrag(qb, stacked_off(R, GT, g, h, ldq), col);
            dor[cc] = ofrag(dob, stacked_off(R, GT, g, h, lddo), col);
        }
        stage_rows(Ql, qr, lane);
        stage_rows(Ol, dor, lane);
        __builtin_amdgcn_wave_barrier();
        int64_t qoff[2], dooff[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            qoff[ti] = stacked_off(i0 + ti * 16 + jl, GT, g, h, ldq);
            dooff[ti] = stacked_off(i0 + ti * 16 + jl, GT, g, h, lddo);
        }
        f32x4 s[2][4], dp[2][4];      // [ti][tj]: query i0 + ti*16 + g4 + r, key j0 + tj*16 + jl
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) s[ti][tj] = dp[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < h; c0 += 32) {
            bf16x8 qa[2], df[2], kf[4], vf[4];
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
                qa[ti] = ofrag(qb, qoff[ti], c0 + c8);
                df[ti] = ofrag(dob, dooff[ti], c0 + c8);
            }
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                kf[tj] = gfrag(kb, ldk, j0 + tj * 16 + jl, T, c0, lane);
                vf[tj] = gfrag(vb, ldv, j0 + tj * 16 + jl, T, c0, lane);
            }
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) {
                    s[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ti], kf[tj], s[ti][tj], 0, 0, 0);
                    dp[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[ti], vf[tj], dp[ti][tj], 0, 0, 0);
                }
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            const float4 Lr = *reinterpret_cast<const float4*>(Lb + i0 + ti * 16 + g4);
            const float4 Dr = *reinterpret_cast<const float4*>(Db + i0 + ti * 16 + g4);
            const float Lv[4] = {Lr.x, Lr.y, Lr.z, Lr.w}, Dv[4] = {Dr.x, Dr.y, Dr.z, Dr.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int R = i0 + ti * 16 + g4 + r;
                const int tr = R < GT ? R / g : -1;
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) {
                    const bool vis = kvis[tj] && j0 + tj * 16 + jl <= tr;
                    const float p = recompute_p(s[ti][tj][r], c, Lv[r]);
                    s[ti][tj][r] = vis ? p : 0.f;
                    dp[ti][tj][r] = vis ? p * (dp[ti][tj][r] - Dv[r]) * scale : 0.f;
                }
            }
        }
        {
            bf16x8 bp[4], bds[4], adot[4], aqt[4];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                bp[tj] = pack_b(s[0][tj], s[1][tj]);
                bds[tj] = pack_b(dp[0][tj], dp[1][tj]);
            }
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                adot[td] = ltfrag(Ol, 0, 16, td * 16, lane);
                aqt[td] = ltfrag(Ql, 0, 16, td * 16, lane);
            }
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) {
                    dvv[td][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adot[td], bp[tj], dvv[td][tj], 0, 0, 0);
                    dk[td][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt[td], bds[tj], dk[td][tj], 0, 0, 0);
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
    store_tile(dk, dk_out + b * T * lddk + (int64_t)kvh * h + slab * AD, lddk, j0, T, lane);
    store_tile(dvv, dv_out + b * T * lddv + (int64_t)kvh * h + slab * AD, lddv, j0, T, lane);
}

// One workgroup per row of the packed buffer.  The q | k columns go through an LDS copy of the row, so the call may run in place:
// every output element of a head depends on two input elements elsewhere in that head.
template <class T>
__global__ __launch_bounds__(256) void gemma_rope_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy,
                                                         const float* __restrict__ table, int64_t rows, int Tn, int qk_heads, int v_cols, int h,
                                                         int inverse) {
    extern __shared__ __attribute__((aligned(16))) char rsm[];
    T* rowl = reinterpret_cast<T*>(rsm);
    const int half = h / 2, qk_cols = qk_heads * h, pairs = qk_heads * half;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const T* xr = x + row * ldx;
        T* yr = y + row * ldy;
        const float* tab = table + (row % Tn) * h;
        for (int cidx = threadIdx.x; cidx < qk_cols; cidx += 256) rowl[cidx] = xr[cidx];
        if (x != y || ldx != ldy)
            for (int cidx = threadIdx.x; cidx < v_cols; cidx += 256) yr[qk_cols + cidx] = xr[qk_cols + cidx];
        __syncthreads();
        for (int p = threadIdx.x; p < pairs; p += 256) {
            const int head = p / half, i = p - head * half;
            const float sn = tab[i], cs = tab[half + i];
            const T* hl = rowl + head * h;
            T* hy = yr + head * h;
            if (!inverse) {
                const float x1 = to_f32(hl[i]), x2 = to_f32(hl[half + i]);
                hy[2 * i] = from_f32<T>(__builtin_fmaf(x1, cs, -(x2 * sn)));
                hy[2 * i + 1] = from_f32<T>(__builtin_fmaf(x2, cs, x1 * sn));
            } else {
                const float ga = to_f32(hl[2 * i]), gb = to_f32(hl[2 * i + 1]);
                hy[i] = from_f32<T>(__builtin_fmaf(ga, cs, gb * sn));
                hy[half + i] = from_f32<T>(__builtin_fmaf(gb, cs, -(ga * sn)));
            }
        }
        __syncthreads();
    }
}

// One workgroup per position of the sorted id list; the one at the head of a run of equal ids owns the run and adds it to that row of dtable
template <class T>
__global__ __launch_bounds__(128) void embedding_grad_kernel(const T* __restrict__ dy, const int64_t* __restrict__ ids, const int64_t* __restrict__ order,
                                                             float* __restrict__ dtable, int64_t n, int64_t vocab, int d, float scale) {
    for (int64_t p = blockIdx.x; p < n; p += gridDim.x) {
        const int64_t id = ids[p];
        if (id < 0 || id >= vocab || (p > 0 && ids[p - 1] == id)) continue;
        for (int col = threadIdx.x; col < d; col += 128) {
            float acc = 0.f;
            for (int64_t e = p; e < n && ids[e] == id; ++e) {
                const int64_t tok = order[e];
                if (tok >= 0 && tok < n) acc += to_f32(dy[tok * d + col]);
            }
            dtable[id * d + col] += acc * scale;
        }
    }
}

bool pitch_ok(int64_t ld, int64_t width) { return ld >= width && ld % 8 == 0; }

}  // namespace

extern "C" int iseg_gemma_rope(const void* qkv, int64_t ld_in, void* out, int64_t ld_out, const float* table, int64_t rows, int T, int nq, int nkv,
                               int h, int inverse, int dtype, hipStream_t stream) {
    const char* who = "iseg_gemma_rope";
    ISEG_REQUIRE(qkv && out && table && rows > 0 && T > 0 && nq > 0 && nkv > 0 && h > 0 && h % 2 == 0 && rows % T == 0, "%s: bad arguments", who);
    const int64_t width = (int64_t)(nq + 2 * nkv) * h, qk = (int64_t)(nq + nkv) * h;
    ISEG_REQUIRE(ld_in >= width && ld_out >= width && width <= INT_MAX, "%s: row pitches must cover (nq + 2 nkv) h = %lld columns", who, (long long)width);
    ISEG_REQUIRE(qk * 4 <= 64 * 1024, "%s: (nq + nkv) h = %lld exceeds the LDS row copy", who, (long long)qk);
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((gemma_rope_kernel<E>), dim3(grid_cap(rows, 1, 65536)), dim3(256), (size_t)qk * sizeof(E), stream, (const E*)qkv, ld_in,
                           (E*)out, ld_out, table, rows, T, nq + nkv, nkv * h, h, inverse);
        return iseg_check_launch(who);
    });
}

extern "C" int iseg_gemma_attention_supported(int nq, int nkv, int h, int dtype) {
    return (dtype == ISEG_BF16 && h >= AD && h <= GH_MAX && h % AD == 0 && nq > 0 && nkv > 0 && nq % nkv == 0) ? 1 : 0;
}

extern "C" size_t iseg_gemma_attention_lse_elems(int64_t batch, int T, int nq, int nkv) {
    if (batch <= 0 || T <= 0 || nq <= 0 || nkv <= 0 || nq % nkv) return 0;
    const int64_t gt = (int64_t)(nq / nkv) * T;
    return (size_t)batch * (size_t)nkv * (size_t)((gt + AQ - 1) / AQ * AQ);
}

#define GEMMA_UNSUPPORTED(cond, ...)          \
    do {                                      \
        if (!(cond)) {                        \
            iseg_set_error(__VA_ARGS__);      \
            return ISEG_ERR_UNSUPPORTED;      \
        }                                     \
    } while (0)

static int gemma_attn_shape_ok(const char* who, int T, int nq, int nkv, int h, float scale, int dtype) {
    GEMMA_UNSUPPORTED(iseg_gemma_attention_supported(nq, nkv, h, dtype),
                      "%s: needs bf16, a head width of 64, 128, 192 or 256 and nq a multiple of nkv (got nq %d, nkv %d, h %d)", who, nq, nkv, h);
    GEMMA_UNSUPPORTED(scale > 0.f && scale <= FLT_MAX, "%s: needs a positive finite scale", who);
    GEMMA_UNSUPPORTED((int64_t)(nq / nkv) * T <= INT_MAX - AQ, "%s: (nq / nkv) * T exceeds the stacked-row index", who);
    return ISEG_OK;
}

extern "C" int iseg_gemma_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                        const uint8_t* padding_mask, void* out, int64_t ldo, float* lse2, int64_t batch, int T, int nq, int nkv,
                                        int h, float scale, int dtype, hipStream_t stream) {
    const char* who = "iseg_gemma_attention_fwd";
    ISEG_REQUIRE(q && k && v && out && batch > 0 && T > 0, "%s: bad arguments", who);
    if (const int rc = gemma_attn_shape_ok(who, T, nq, nkv, h, scale, dtype)) return rc;
    GEMMA_UNSUPPORTED(pitch_ok(ldq, (int64_t)nq * h) && pitch_ok(ldk, (int64_t)nkv * h) && pitch_ok(ldv, (int64_t)nkv * h) &&
                          pitch_ok(ldo, (int64_t)nq * h),
                      "%s: row pitches must be multiples of 8 elements and cover their rows (got %lld %lld %lld %lld)", who, (long long)ldq,
                      (long long)ldk, (long long)ldv, (long long)ldo);
    GEMMA_UNSUPPORTED(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)lse2) % 16 == 0,
                      "%s: operands must be 16-byte aligned", who);
    const int g = nq / nkv, qtiles = (g * T + AQ - 1) / AQ;
    const int64_t items = batch * nkv * qtiles * (h / AD);
    ISEG_REQUIRE(items <= INT_MAX, "%s: too many work items", who);
    hipLaunchKernelGGL(gemma_attn_fwd_kernel, dim3((unsigned)items), dim3(64), 0, stream, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk,
                       (const bf16_t*)v, ldv, padding_mask, (bf16_t*)out, ldo, lse2, T, nkv, g, h, qtiles, scale);
    return iseg_check_launch(who);
}

extern "C" int iseg_gemma_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                        const uint8_t* padding_mask, const void* out, int64_t ldo, const void* dout, int64_t lddo,
                                        const float* lse2, float* dsum, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                        int64_t batch, int T, int nq, int nkv, int h, float scale, int dtype, hipStream_t stream) {
    const char* who = "iseg_gemma_attention_bwd";
    ISEG_REQUIRE(q && k && v && out && dout && lse2 && dsum && dq && dk && dv && batch > 0 && T > 0, "%s: bad arguments", who);
    if (const int rc = gemma_attn_shape_ok(who, T, nq, nkv, h, scale, dtype)) return rc;
    const int64_t wq = (int64_t)nq * h, wk = (int64_t)nkv * h;
    GEMMA_UNSUPPORTED(pitch_ok(ldq, wq) && pitch_ok(ldk, wk) && pitch_ok(ldv, wk) && pitch_ok(ldo, wq) && pitch_ok(lddo, wq) &&
                          pitch_ok(lddq, wq) && pitch_ok(lddk, wk) && pitch_ok(lddv, wk),
                      "%s: row pitches must be multiples of 8 elements and cover their rows", who);
    GEMMA_UNSUPPORTED(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)lse2 | (uintptr_t)dsum |
                       (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % 16 == 0,
                      "%s: operands must be 16-byte aligned", who);
    const int g = nq / nkv, qtiles = (g * T + AQ - 1) / AQ, ktiles = (T + AK - 1) / AK, slabs = h / AD;
    const int Tp = qtiles * AQ;
    const int64_t qitems = batch * nkv * qtiles * slabs, kitems = batch * nkv * ktiles * slabs, rows = batch * T * nq;
    ISEG_REQUIRE(qitems <= INT_MAX && kitems <= INT_MAX && ceil_div64(rows * 8, 256) <= INT_MAX, "%s: too many work items", who);
    const bf16_t *qp = (const bf16_t*)q, *kp = (const bf16_t*)k, *vp = (const bf16_t*)v, *dop = (const bf16_t*)dout;
    (void)hipMemsetAsync(dsum, 0, iseg_gemma_attention_lse_elems(batch, T, nq, nkv) * sizeof(float), stream);      // the padding rows are read
    hipLaunchKernelGGL(gemma_attn_rowdot_kernel, dim3((unsigned)ceil_div64(rows * 8, 256)), dim3(256), 0, stream, (const bf16_t*)out, ldo, dop,
                       lddo, dsum, rows, T, nq, g, h, Tp);
    hipLaunchKernelGGL(gemma_attn_dq_kernel, dim3((unsigned)qitems), dim3(64), 0, stream, qp, ldq, kp, ldk, vp, ldv, padding_mask, dop, lddo, lse2,
                       dsum, (bf16_t*)dq, lddq, T, nkv, g, h, qtiles, scale);
    hipLaunchKernelGGL(gemma_attn_dkv_kernel, dim3((unsigned)kitems), dim3(64), 0, stream, qp, ldq, kp, ldk, vp, ldv, padding_mask, dop, lddo, lse2,
                       dsum, (bf16_t*)dk, lddk, (bf16_t*)dv, lddv, T, nkv, g, h, ktiles, Tp, scale);
    return iseg_check_launch(who);
}

extern "C" int iseg_embedding_grad(const void* dy, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n, int64_t vocab, int d,
                                   float scale, int dtype, hipStream_t stream) {
    const char* who = "iseg_embedding_grad";
    ISEG_REQUIRE(dy && sorted_ids && order && dtable && n > 0 && vocab > 0 && d > 0, "%s: bad arguments", who);
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((embedding_grad_kernel<E>), dim3(grid_cap(n, 1, 65536)), dim3(128), 0, stream, (const E*)dy, sorted_ids, order, dtable, n,
                           vocab, d, scale);
        return iseg_check_launch(who);
    });
}
