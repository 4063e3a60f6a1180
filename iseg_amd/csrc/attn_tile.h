// The online-softmax attention core shared by flashattn.hip (packed [q|k|v], heads x 64) and selfattn.hip (one head, 64-wide
// query / key, value slabs of 64 columns), and the MFMA fragment helpers these two share with winattn.hip.
//
// One wavefront owns 64 rows of one problem and walks the other side in tiles, v_mfma_f32_16x16x32_bf16 throughout.  A fragment
// (A or B operand) = lane holds 8 consecutive k = 8 * (lane >> 4) .. + 7 of row (or column) lane & 15; the accumulator holds
// D[(lane >> 4) * 4 + r][lane & 15], r = 0..3.  The tile bodies take base pointers and row pitches of ONE problem (sample, head,
// value slab): how a work item becomes those is the business of the kernel that calls them.  Nothing of size T x T is ever
// stored; no atomics, fixed summation order.
//   * attn_fwd_tile -- 64 queries, key tiles of 64, transposed orientation: S^T = K Q^T (keys on MFMA rows, queries on columns), so
//     each lane owns ONE query column per 16-wide query tile and sixteen of its 64 keys: the row max / row sum are 15 in-lane ops
//     + two cross-group exchanges, the running (m, l, alpha) are one scalar per query tile, and the probabilities are already laid
//     out as the B operand of O^T = V^T P^T (k slots = the lane's own keys; the V^T fragment is gathered to match) -- P never
//     touches LDS.  Also returns L[i] = log2 sum_j exp2(c * s_ij), c = scale * log2 e.
//   * (the dQ kernels keep a body each, built from the helpers below: through one body with the dP^T = V dO^T product as a
//     policy the streamed form of selfattn.hip measured 1.7 % slower, EXPERIMENTS.md)
//   * attn_key_tile -- 64 keys, query rows 32 at a time, natural orientation: S = Q K^T, dP = dO V^T; P and dS are the B operands
//     of dV^T = dO^T P and dK^T = Q^T dS, dO^T / Q^T gathered from their LDS images.
// Rows >= T are never read (zero fragments) and never stored.
#pragma once
#include "common.h"

#include <float.h>

namespace attn {

typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;

constexpr int AD = 64;         // query / key width, and the width of one value slab
constexpr int AQ = 64;         // query rows per wavefront (forward, dQ)
constexpr int AK = 64;         // keys per tile
constexpr int AI = 32;         // query rows per inner step of the key-owning body (one MFMA k-step): keeps it inside 512 VGPRs
constexpr int ASTRIDE = 72;    // LDS image row stride (bf16): 144-B rows
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
    return v;
}
// MFMA A / B operand fragment straight from global memory: row `row` (zeros past T), columns col0 + 8 * (lane / 16) .. + 7
__device__ __forceinline__ bf16x8 gfrag(const bf16_t* __restrict__ base, int64_t ld, int row, int T, int col0, int lane) {
    if (row >= T) return zero8();
    return *reinterpret_cast<const bf16x8*>(base + (int64_t)row * ld + col0 + 8 * (lane >> 4));
}
// staging chunk of a tile row (zeros past T)
__device__ __forceinline__ bf16x8 grow8(const bf16_t* __restrict__ base, int64_t ld, int row, int T, int col) {
    if (row >= T) return zero8();
    return *reinterpret_cast<const bf16x8*>(base + (int64_t)row * ld + col);
}
// fragment from a row-major LDS image read along the rows: row r0 + (lane & 15), k0 + 8 * (lane >> 4) .. + 7   (one ds_read_b128)
__device__ __forceinline__ bf16x8 row_frag(const bf16_t* lds, int stride, int r0, int k0, int lane) {
    return *reinterpret_cast<const bf16x8*>(lds + (r0 + (lane & 15)) * stride + k0 + 8 * (lane >> 4));
}
// transposed fragment (A operand) for columns c0 .. c0+15 of an LDS image [row][ASTRIDE]: this lane's eight k slots are the rows
// rowA + 4g + 0..3 and rowB + 4g + 0..3 -- the same row set its accumulators of the preceding product hold
__device__ __forceinline__ bf16x8 ltfrag(const bf16_t* lds, int rowA, int rowB, int c0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(lds + (rowA + 4 * g + q) * ASTRIDE + c0 + 4 * p));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(lds + (rowB + 4 * g + q) * ASTRIDE + c0 + 4 * p));
    bf16x8 f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[i] = lo[i];
        f[4 + i] = hi[i];
    }
    return f;
}
__device__ __forceinline__ float xorf(float v, int mask) { return __shfl_xor(v, mask, 64); }

// N * 8 staged rows of a 64-column tile, registers -> LDS image: chunk = lane + 64 * cc -> row (lane >> 3) + 8 * cc
template <int N>
__device__ __forceinline__ void stage_rows(bf16_t* img, const bf16x8 (&regs)[N], int lane) {
#pragma unroll
    for (int cc = 0; cc < N; ++cc) *reinterpret_cast<bf16x8*>(img + ((lane >> 3) + 8 * cc) * ASTRIDE + (lane & 7) * 8) = regs[cc];
}
// two accumulator tiles -> one B operand: k slots 0..3 from `lo`, 4..7 from `hi` (the row sets ltfrag gathers)
__device__ __forceinline__ bf16x8 pack_b(const f32x4& lo, const f32x4& hi) {
    bf16x8 b;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        b[r] = (bf16_t)lo[r];
        b[4 + r] = (bf16_t)hi[r];
    }
    return b;
}
__device__ __forceinline__ void zero_tiles(f32x4 (&a)[4][4]) {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) a[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// probability recomputed from the score and the row's log2-sum-exp
__device__ __forceinline__ float recompute_p(float s, float c, float L) { return __builtin_amdgcn_exp2f(__builtin_fmaf(s, c, -L)); }
// acc[td][t] holds rows row0 + t*16 + (lane & 15), columns td*16 + (lane >> 4) * 4 + r of a 64 x 64 tile: rows below T are stored
__device__ __forceinline__ void store_tile(const f32x4 (&acc)[4][4], bf16_t* __restrict__ base, int64_t ld, int row0, int T, int lane) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row = row0 + t * 16 + (lane & 15);
        if (row < T) {
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16_t)acc[td][t][r];
                *reinterpret_cast<bf16x4*>(base + (int64_t)row * ld + td * 16 + (lane >> 4) * 4) = w;
            }
        }
    }
}

// Forward for query tile qt.  K fragments come straight from global memory (16 B per lane, prefetched one tile ahead), V goes
// through the wave-private LDS image Vl [AK][ASTRIDE] and ds_read_b64_tr_b16.  The output tile is columns ocol .. ocol + 63 of
// ob.  lse_row: this problem's row of L, padded to a multiple of 64 (zeros past T), written only with want_lse (training, and
// one value slab per row) and not touched otherwise.  Keys past T in the ragged last tile get the score -FLT_MAX; with
// ZERO_PAST_T their probability is also set to exactly 0, without it the exp2 underflow is relied on.
// The schedule of this body is touchy: with the V staging through helpers like stage_rows, with the output column folded into
// ob, or with a null lse_row in place of the flag, one of the two forward kernels measured about 2 % slower (EXPERIMENTS.md).
template <bool ZERO_PAST_T>
__device__ __forceinline__ void attn_fwd_tile(const bf16_t* qb, int64_t ldq, const bf16_t* kb, int64_t ldk,
                                              const bf16_t* vb, int64_t ldv, bf16_t* ob, int64_t ldo, int ocol,
                                              float* lse_row, bool want_lse, int qt, int T, float scale, bf16_t* Vl, int lane) {
    const int q0 = qt * AQ;
    const int jl = lane & 15, g4 = (lane >> 4) * 4;
    const float c = scale * LOG2E;
    const int vrow = lane >> 3, vcol = (lane & 7) * 8;

    bf16x8 aq[4][2], kf[4][2], vr[8];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) aq[ti][ks] = gfrag(qb, ldq, q0 + ti * 16 + jl, T, ks * 32, lane);
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) kf[tj][ks] = gfrag(kb, ldk, tj * 16 + jl, T, ks * 32, lane);
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) vr[cc] = grow8(vb, ldv, vrow + 8 * cc, T, vcol);

    f32x4 o[4][4];      // [td][ti]: O[i = ti*16 + jl][dd = td*16 + g4 + r]
    float m[4], l[4];
    zero_tiles(o);
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        m[ti] = -FLT_MAX;
        l[ti] = 0.f;
    }

    for (int k0 = 0; k0 < T; k0 += AK) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) *reinterpret_cast<bf16x8*>(Vl + (vrow + 8 * cc) * ASTRIDE + vcol) = vr[cc];
        f32x4 s[4][4];      // [tj][ti]: S[i = ti*16 + jl][key = k0 + tj*16 + g4 + r]
        zero_tiles(s);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) s[tj][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[tj][ks], aq[ti][ks], s[tj][ti], 0, 0, 0);
        // next tile's K fragments and V rows start their trip now; they land while this tile's softmax and P V run
        if (k0 + AK < T) {
            const int n0 = k0 + AK;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) kf[tj][ks] = gfrag(kb, ldk, n0 + tj * 16 + jl, T, ks * 32, lane);
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) vr[cc] = grow8(vb, ldv, n0 + vrow + 8 * cc, T, vcol);
        }
        const bool ragged = k0 + AK > T;
        if (ragged) {      // keys past T stay out of the row maximum
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + tj * 16 + g4 + r >= T) {
#pragma unroll
                        for (int ti = 0; ti < 4; ++ti) s[tj][ti][r] = -FLT_MAX;
                    }
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
            float mx = s[0][ti][0];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[tj][ti][r]);
            mx = fmaxf(mx, xorf(mx, 16));
            mx = fmaxf(mx, xorf(mx, 32));
            const float mnew = fmaxf(m[ti], mx);
            const float alpha = __builtin_amdgcn_exp2f((m[ti] - mnew) * c);
            const float mc = mnew * c;
            m[ti] = mnew;
            float sum = 0.f;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pv = recompute_p(s[tj][ti][r], c, mc);
                    if (ZERO_PAST_T && ragged && k0 + tj * 16 + g4 + r >= T) pv = 0.f;
                    s[tj][ti][r] = pv;
                    sum += pv;
                }
            l[ti] = l[ti] * alpha + sum;      // per-lane partial over this lane's keys; the four key groups are summed once at the end
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
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bp[ti][r] = (bf16_t)s[2 * ks][ti][r];
                    bp[ti][4 + r] = (bf16_t)s[2 * ks + 1][ti][r];
                }
#pragma unroll
            for (int td = 0; td < 4; ++td) av[td] = ltfrag(Vl, 32 * ks, 32 * ks + 16, td * 16, lane);
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti) o[td][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[td], bp[ti], o[td][ti], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        float lt = l[ti];
        lt += xorf(lt, 16);
        lt += xorf(lt, 32);
        const float inv = __frcp_rn(lt);
        const int i = q0 + ti * 16 + jl;
        // training: log2 of the softmax denominator in the exp2 domain of this body
        if (want_lse && g4 == 0) lse_row[i] = i < T ? __builtin_fmaf(m[ti], c, __log2f(lt)) : 0.f;
        if (i < T) {
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16_t)(o[td][ti][r] * inv);
                *reinterpret_cast<bf16x4*>(ob + (int64_t)i * ldo + ocol + td * 16 + g4) = w;
            }
        }
    }
}

// Key side for key tile kt: dK (DK) and / or dV (DV) of 64 keys, the query rows walked AI = 32 at a time; Lb / Db are this
// problem's rows of L and D.  Ql / Ol are the wave-private images [AI][ASTRIDE] of the step's Q and dO rows: dK needs Q^T from
// Ql, dV needs dO^T from Ol; without DK the Q fragments of S come straight from global memory, one step ahead.  dob / dvb point
// at the 64 columns dV is asked for.  The dP = dO V^T product of dK, NARROW (dv == 64): V fragments held for the whole loop, dO
// fragments from Ol (which then must be staged: DV); otherwise both streamed over a run-time dv, 32 columns per step.  MASK switches
// query rows and keys past T off explicitly; without it the zero q / dO rows past T make their terms vanish (as long as
// exp2(c * s - L) stays finite there) and key columns past T are never stored.
template <bool DK, bool DV, bool NARROW, bool MASK>
__device__ __forceinline__ void attn_key_tile(const bf16_t* __restrict__ qb, int64_t ldq, const bf16_t* __restrict__ kb, int64_t ldk,
                                              const bf16_t* __restrict__ vb, int64_t ldv, const bf16_t* __restrict__ dob, int64_t lddo,
                                              const float* __restrict__ Lb, const float* __restrict__ Db, bf16_t* __restrict__ dkb,
                                              int64_t lddk, bf16_t* __restrict__ dvb, int64_t lddv, int kt, int T, int dv, float scale,
                                              bf16_t* Ql, bf16_t* Ol, int lane) {
    static_assert(!NARROW || (DK && DV), "the narrow dP product reads the dO image that dV stages");
    const int j0 = kt * AK;
    const int jl = lane & 15, g4 = (lane >> 4) * 4;
    const float c = scale * LOG2E;

    bf16x8 kfB[4][2], vfB[4][2], qr[4], dor[4], qn[2][2];      // vfB: NARROW; qr: DK; dor: DV; qn: !DK
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kfB[tj][ks] = gfrag(kb, ldk, j0 + tj * 16 + jl, T, ks * 32, lane);
            if constexpr (NARROW) vfB[tj][ks] = gfrag(vb, ldv, j0 + tj * 16 + jl, T, ks * 32, lane);
        }
    auto fetch = [&](int i0) {
        if constexpr (!DK) {
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) qn[ti][ks] = gfrag(qb, ldq, i0 + ti * 16 + jl, T, ks * 32, lane);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int row = i0 + (lane >> 3) + 8 * cc, col = (lane & 7) * 8;
            const bool ok = row < T;      // one test for both rows
            if constexpr (DK) qr[cc] = ok ? *reinterpret_cast<const bf16x8*>(qb + (int64_t)row * ldq + col) : zero8();
            if constexpr (DV) dor[cc] = ok ? *reinterpret_cast<const bf16x8*>(dob + (int64_t)row * lddo + col) : zero8();
        }
    };
    fetch(0);
    f32x4 dk[4][4], dvv[4][4];      // [td][tj]: key j0 + tj*16 + jl, column td*16 + g4 + r
    zero_tiles(dk);
    zero_tiles(dvv);

    for (int i0 = 0; i0 < T; i0 += AI) {
        bf16x8 qf[2][2];
        if constexpr (!DK) {
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) qf[ti][ks] = qn[ti][ks];
        }
        if constexpr (DK) stage_rows(Ql, qr, lane);
        if constexpr (DV) stage_rows(Ol, dor, lane);
        __builtin_amdgcn_wave_barrier();
        if (i0 + AI < T) fetch(i0 + AI);      // next step's rows fly during this step's MFMAs
        f32x4 s[2][4], dp[2][4];      // [ti][tj]: query i0 + ti*16 + g4 + r, key j0 + tj*16 + jl
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) s[ti][tj] = dp[ti][tj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti) {
                bf16x8 qa, df;
                if constexpr (DK) qa = row_frag(Ql, ASTRIDE, ti * 16, ks * 32, lane);
                else qa = qf[ti][ks];
                if constexpr (NARROW) df = row_frag(Ol, ASTRIDE, ti * 16, ks * 32, lane);
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) {
                    s[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kfB[tj][ks], s[ti][tj], 0, 0, 0);
                    if constexpr (NARROW) dp[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, vfB[tj][ks], dp[ti][tj], 0, 0, 0);
                }
            }
        if constexpr (DK && !NARROW) {
#pragma unroll 2
            for (int c0 = 0; c0 < dv; c0 += 32) {
                bf16x8 ds[2], vs[4];
#pragma unroll
                for (int ti = 0; ti < 2; ++ti) ds[ti] = gfrag(dob, lddo, i0 + ti * 16 + jl, T, c0, lane);
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) vs[tj] = gfrag(vb, ldv, j0 + tj * 16 + jl, T, c0, lane);
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int tj = 0; tj < 4; ++tj) dp[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ds[ti], vs[tj], dp[ti][tj], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            const float4 Lr = *reinterpret_cast<const float4*>(Lb + i0 + ti * 16 + g4);
            float4 Dr = {0.f, 0.f, 0.f, 0.f};
            if constexpr (DK) Dr = *reinterpret_cast<const float4*>(Db + i0 + ti * 16 + g4);
            const float Lv[4] = {Lr.x, Lr.y, Lr.z, Lr.w}, Dv[4] = {Dr.x, Dr.y, Dr.z, Dr.w};
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                const bool keyoff = MASK && j0 + tj * 16 + jl >= T;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool off = MASK && (keyoff || i0 + ti * 16 + g4 + r >= T);
                    const float p = recompute_p(s[ti][tj][r], c, Lv[r]);
                    if constexpr (DV) s[ti][tj][r] = off ? 0.f : p;
                    if constexpr (DK) {
                        const float dsv = p * (dp[ti][tj][r] - Dv[r]) * scale;
                        dp[ti][tj][r] = off ? 0.f : dsv;
                    }
                }
            }
        }
        {
            bf16x8 bp[4], bds[4], adot[4], aqt[4];
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                if constexpr (DV) bp[tj] = pack_b(s[0][tj], s[1][tj]);
                if constexpr (DK) bds[tj] = pack_b(dp[0][tj], dp[1][tj]);
            }
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                if constexpr (DV) adot[td] = ltfrag(Ol, 0, 16, td * 16, lane);
                if constexpr (DK) aqt[td] = ltfrag(Ql, 0, 16, td * 16, lane);
            }
#pragma unroll
            for (int td = 0; td < 4; ++td)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) {
                    if constexpr (DV) dvv[td][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(adot[td], bp[tj], dvv[td][tj], 0, 0, 0);
                    if constexpr (DK) dk[td][tj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aqt[td], bds[tj], dk[td][tj], 0, 0, 0);
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (DK) store_tile(dk, dkb, lddk, j0, T, lane);
    if constexpr (DV) store_tile(dvv, dvb, lddv, j0, T, lane);
}

}  // namespace attn
