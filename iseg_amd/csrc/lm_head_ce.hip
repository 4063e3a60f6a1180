// Chunked-vocabulary cross-entropy of the language-model head (SparseCategoricalCrossentropy(from_logits=True) + SparseCategoricalAccuracy behind
// nlp/gemma/gemma_causal.py:165-172): the logits  Z = X E^T  [M, V] are never stored.  The caller walks the tied table E in chunks of columns; for
// each chunk the GEMM launcher writes  Z_c [M, w]  in fp32 and the kernels here consume it while it is hot.  include/iseg_hip.h has the full
// statement; in short
//   chunk_fwd   per row an online softmax state (m, s, z_t, first-maximal index) is merged with the chunk
//   target_logit  z_t once more as the fp64 dot product x_r . E[t_r], rounded once (the loss carries this one logit's error whole)
//   finalise    per row  lse = m + log s,  loss = w_row (lse - z_t),  match = (argmax == t);  three sums over rows in a fixed order
//   chunk_bwd   G_c = scale w_row up_row (exp(z - m) / s - onehot), rounded once to the compute dtype, from the RECOMPUTED Z_c
// One wavefront owns one row of a chunk: a lane walks it in 16-byte pieces with four loads in flight (4 KiB of the row per wave step), the lanes'
// partial states are merged by a butterfly of wavefront shuffles.  Four rows per 256-thread workgroup; at M in the thousands that is eight
// workgroups = 32 wavefronts per CU on a 256-CU chip.  The vocabulary is not split across workgroups and nothing is added with atomics: a second
// call returns the same bits.
#include "common.h"
#include "iseg_hip.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LH_THREADS = 256;
constexpr int LH_ROWS = LH_THREADS / 64;      // rows (wavefronts) per workgroup
constexpr int LH_UNROLL = 4;                  // 16-byte loads a lane has in flight
constexpr int LH_STEP = 64 * 4 * LH_UNROLL;   // elements of a row per wave step
constexpr int LH_FIN_ROWS = 256;              // rows per workgroup of the finalise pass: one partial record of three sums each
constexpr int64_t LH_GRID_CAP = 8192;         // workgroups of the chunk kernels; rows beyond are taken in further trips
constexpr float LH_LOG2E = 1.4426950408889634f;       // log2 e rounded to fp32 ...
constexpr float LH_LOG2E_LO = 1.925963033500011e-8f;  // ... and what the rounding dropped
constexpr float LH_LN2 = 0.6931471805599453f;

// exp(t) for t <= 0 (or -inf, or NaN) to v_exp_f32's one ulp whatever |t| is: t log2 e = hi + lo with the product's rounding error and the
// constant's in lo, exp2(hi) (1 + lo ln 2).  With the product rounded once alone the result is off by 2^-24 |t|, which at the fp32 compute type is
// what decides between this route and the stored-logits one.  exp(-inf) = 0 (not 0 * NaN); NaN stays NaN.
__device__ __forceinline__ float exp_neg(float t) {
    const float hi = t * LH_LOG2E;
    const float lo = fmaf(t, LH_LOG2E, -hi) + t * LH_LOG2E_LO;
    const float e = __builtin_amdgcn_exp2f(hi);
    return e == 0.f ? 0.f : fmaf(e, lo * LH_LN2, e);
}

// the reference point of the exponentials: the running maximum, or 0 while it is still -inf (x - (-inf) would be NaN for x = -inf)
__device__ __forceinline__ float ref_of(float m) { return m == -INFINITY ? 0.f : m; }

// four elements of a row from column i0 on; columns at or past w read as -inf (weight 0, never the maximum)
__device__ __forceinline__ void load4(const float* __restrict__ row, int i0, int w, bool vec, float (&x)[4]) {
    if (vec && i0 + 3 < w) {
        const float4 q = *reinterpret_cast<const float4*>(row + i0);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = i0 + j < w ? row[i0 + j] : -INFINITY;
    }
}

// blockIdx.x * LH_ROWS + wave = first row; rows stride by gridDim.x * LH_ROWS
__global__ __launch_bounds__(LH_THREADS) void lm_head_ce_chunk_fwd_kernel(const float* __restrict__ z, int64_t ld, const int32_t* __restrict__ targets,
                                                                          float* __restrict__ m_state, float* __restrict__ s_state,
                                                                          float* __restrict__ zt_state, int32_t* __restrict__ arg_state, int64_t M,
                                                                          int v0, int w, int vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * LH_ROWS + wave; r < M; r += (int64_t)gridDim.x * LH_ROWS) {
        const float* row = z + r * ld;
        float m = -INFINITY, s = 0.f;      // of this lane's columns
        int arg = INT_MAX;
        for (int i0 = lane * 4; i0 < w; i0 += LH_STEP) {
            float x[LH_UNROLL][4];
#pragma unroll
            for (int u = 0; u < LH_UNROLL; ++u) load4(row, i0 + u * 256, w, vec != 0, x[u]);
            float mx = m;      // columns are visited in increasing order: a strict compare keeps the smallest index of equal values
#pragma unroll
            for (int u = 0; u < LH_UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x[u][j] > mx) mx = x[u][j], arg = i0 + u * 256 + j;
            if (mx > m) {
                s *= exp_neg(m - mx);      // m = -inf: s is 0 and stays 0
                m = mx;
            }
            const float ref = ref_of(m);
#pragma unroll
            for (int u = 0; u < LH_UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) s += exp_neg(x[u][j] - ref);      // a NaN column makes s NaN: the row's loss is NaN
        }
        // the lanes' states: the maximum with its smallest column, then the sums moved to it
        float cm = m;
        int carg = arg;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const float om = __shfl_xor(cm, off);
            const int oa = __shfl_xor(carg, off);
            if (om > cm || (om == cm && oa < carg)) cm = om, carg = oa;
        }
        // (the 64 partial sums and the merge with the state in fp64: per row, not per element; the state is rounded once per chunk)
        double cs = (double)s * (double)exp_neg(m - ref_of(cm));
#pragma unroll
        for (int off = 32; off; off >>= 1) cs += __shfl_xor(cs, off);
        if (lane == 0) {
            const float m0 = m_state[r], s0 = s_state[r];
            const float mn = cm > m0 ? cm : m0, ref = ref_of(mn);
            m_state[r] = mn;
            s_state[r] = (float)((double)s0 * (double)exp_neg(m0 - ref) + cs * (double)exp_neg(cm - ref));
            if (cm > m0) arg_state[r] = v0 + carg;      // strict: an earlier chunk keeps a tie
            const int t = targets[r];
            if (t >= v0 && t - v0 < w) zt_state[r] = row[t - v0];
        }
    }
}

// z_t once more, as the dot product x_r . E[t_r] summed in fp64 and rounded once.  The loss is ONE logit against a softmax-weighted average of
// all of them: the average smooths the GEMM's accumulation error (d roundings per logit), the single logit carries it whole -- measured, it is
// what separates the fp32 loss from the correctly rounded one.  M d multiply-adds, one wavefront per row, eight elements per lane and step.
template <class T>
__global__ __launch_bounds__(LH_THREADS) void lm_head_ce_target_logit_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ table,
                                                                             int64_t ldt, const int32_t* __restrict__ targets,
                                                                             float* __restrict__ zt_state, int64_t M, int V, int d, int vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * LH_ROWS + wave; r < M; r += (int64_t)gridDim.x * LH_ROWS) {
        const int t = targets[r];
        if (t < 0 || t >= V) continue;      // wave-uniform: the row has no class and its z_t is not read
        const T* a = x + r * ldx;
        const T* b = table + (int64_t)t * ldt;
        double acc = 0.0;
        if (vec) {
            for (int k = lane * 8; k < d; k += 64 * 8) {
                float u[8], v[8];
                load8<T>(a + k, u);
                load8<T>(b + k, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc += (double)u[j] * (double)v[j];
            }
        } else {
            for (int k = lane; k < d; k += 64) acc += (double)to_f32(a[k]) * (double)to_f32(b[k]);
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) zt_state[r] = (float)acc;
    }
}

// per-row outputs and, per workgroup of LH_FIN_ROWS rows, one record (sum loss, sum w match, sum w) summed in lane / wave order
__global__ __launch_bounds__(LH_FIN_ROWS) void lm_head_ce_finalise_kernel(const float* __restrict__ m_state, const float* __restrict__ s_state,
                                                                          const float* __restrict__ zt_state, const int32_t* __restrict__ arg_state,
                                                                          const int32_t* __restrict__ targets, const float* __restrict__ weights,
                                                                          float* __restrict__ loss, float* __restrict__ lse, int32_t* __restrict__ match,
                                                                          float* __restrict__ partials, int64_t M, int V, float scale) {
    __shared__ float red[LH_FIN_ROWS / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * LH_FIN_ROWS + threadIdx.x;
    float l = 0.f, wm = 0.f, wr = 0.f;
    if (r < M) {
        const int t = targets[r];
        const bool valid = t >= 0 && t < V;
        wr = valid ? (weights ? weights[r] : 1.f) : 0.f;
        // one row per thread, once per call: fp64, rounded once.  (In fp32 it would be log s - (z_t - m), not (m + log s) - z_t, as in the
        // loss kernel of loss.hip: with large logits m + log s is rounded at their magnitude.)
        const double mx = (double)m_state[r], ls = log((double)s_state[r]);
        const float e = (float)(mx + ls);
        const bool hit = valid && arg_state[r] == t;
        // a row of weight 0 (or without a class) costs exactly 0 whatever its logits hold
        l = wr == 0.f ? 0.f : (float)((double)scale * (double)wr * (ls - ((double)zt_state[r] - mx)));
        wm = hit ? wr : 0.f;
        loss[r] = l;
        lse[r] = e;
        match[r] = hit ? 1 : 0;
    }
    l = wave_sum(l), wm = wave_sum(wm), wr = wave_sum(wr);
    if (lane == 0) red[wave][0] = l, red[wave][1] = wm, red[wave][2] = wr;
    __syncthreads();
    if (threadIdx.x < 3) {
        float t = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < LH_FIN_ROWS / 64; ++k) t += red[k][threadIdx.x];
        partials[(int64_t)blockIdx.x * 3 + threadIdx.x] = t;
    }
}

// one workgroup: thread i sums the records i, i + 256, ... in order (fp64), then lanes, then waves
__global__ __launch_bounds__(256) void lm_head_ce_sums_kernel(const float* __restrict__ partials, int64_t n, float* __restrict__ sums) {
    __shared__ double red[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] += (double)partials[i * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off; off >>= 1) a[k] += __shfl_xor(a[k], off);
        if (lane == 0) red[wave][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) sums[threadIdx.x] = (float)(((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]);
}

// a lane owns eight consecutive columns per wave step: two 16-byte loads of z, one 16-byte (bf16) or two (fp32) stores of G
template <class T>
__global__ __launch_bounds__(LH_THREADS) void lm_head_ce_chunk_bwd_kernel(const float* __restrict__ z, int64_t ld, const float* __restrict__ m_state,
                                                                          const float* __restrict__ s_state, const int32_t* __restrict__ targets, const float* __restrict__ weights,
                                                                          const float* __restrict__ upstream, float scale, T* __restrict__ g,
                                                                          int64_t ldg, int64_t M, int V, int v0, int w, int vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * LH_ROWS + wave; r < M; r += (int64_t)gridDim.x * LH_ROWS) {
        const float* row = z + r * ld;
        T* out = g + r * ldg;
        const int t = targets[r];
        const bool valid = t >= 0 && t < V;
        const float wr = valid ? (weights ? weights[r] : 1.f) : 0.f;
        const bool dead = wr == 0.f;      // zeros, not NaN * 0: the row's logits are not read
        // the row's factor and factor / s, each rounded once: G = e (coef / s) - [hot] coef
        const double coef64 = dead ? 0.0 : (double)scale * (double)wr * (upstream ? (double)upstream[r] : 1.0);
        const float coef = (float)coef64;
        // softmax as exp(z - m) / s, not exp(z - (m + log s)): the sum m + log s is rounded at ITS magnitude and would move every
        // probability of the row by that; z - m is exact for neighbouring magnitudes
        const float mx = dead ? 0.f : m_state[r];
        const float cinv = dead ? 0.f : (float)(coef64 / (double)s_state[r]);
        const int hot = valid ? t - v0 : -1;
        for (int i0 = lane * 8; i0 < w; i0 += 64 * 8) {
            float y[8];
            if (dead) {
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] = 0.f;
            } else {
                float x[2][4];
                load4(row, i0, w, vec != 0, x[0]);
                load4(row, i0 + 4, w, vec != 0, x[1]);
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] = exp_neg(x[j >> 2][j & 3] - mx) * cinv - (i0 + j == hot ? coef : 0.f);
            }
            if (vec && i0 + 7 < w) {
                store8<T>(out + i0, y);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (i0 + j < w) out[i0 + j] = from_f32<T>(y[j]);
            }
        }
    }
}

int64_t fin_blocks(int64_t M) { return ceil_div64(M, LH_FIN_ROWS); }

}  // namespace

extern "C" int iseg_lm_head_ce_chunk_default(int64_t M, int64_t V) {
    // profiles/lm_head_ce_kbench.md: the step's time is flat in the chunk width from 4096 up; 8192 keeps Z_c and G_c of 8192 rows at 384 MiB
    (void)M;
    if (V < 1) return 0;
    return (int)(V < 8192 ? V : 8192);
}

extern "C" size_t iseg_lm_head_ce_scratch_bytes(int64_t M) { return M < 1 ? 0 : (size_t)fin_blocks(M) * 3 * sizeof(float); }

extern "C" int iseg_lm_head_ce_chunk_fwd(const float* z, int64_t ld, const int32_t* targets, float* m, float* s, float* zt, int32_t* argmax,
                                         int64_t M, int64_t v0, int64_t w, hipStream_t stream) {
    const char* who = "iseg_lm_head_ce_chunk_fwd";
    ISEG_REQUIRE(z && targets && m && s && zt && argmax && M > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(w >= 1 && v0 >= 0 && v0 + w <= INT_MAX - LH_STEP, "%s: the chunk [%lld, %lld) is empty or past 2^31", who, (long long)v0,
                 (long long)(v0 + w));
    ISEG_REQUIRE(ld >= w, "%s: the row pitch %lld does not cover %lld columns", who, (long long)ld, (long long)w);
    const int vec = (uintptr_t)z % 16 == 0 && ld % 4 == 0;
    hipLaunchKernelGGL(lm_head_ce_chunk_fwd_kernel, dim3(grid_cap(M, LH_ROWS, LH_GRID_CAP)), dim3(LH_THREADS), 0, stream, z, ld, targets, m, s, zt, argmax,
                       M, (int)v0, (int)w, vec);
    return iseg_check_launch(who);
}

extern "C" int iseg_lm_head_ce_target_logit(const void* x, int64_t ldx, const void* table, int64_t ldt, const int32_t* targets, float* zt, int64_t M,
                                            int64_t V, int64_t d, int dtype, hipStream_t stream) {
    const char* who = "iseg_lm_head_ce_target_logit";
    ISEG_REQUIRE(x && table && targets && zt && M > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(V >= 1 && V <= INT_MAX && d >= 1 && d <= INT_MAX - 64 * 8, "%s: bad sizes V %lld d %lld", who, (long long)V, (long long)d);
    ISEG_REQUIRE(ldx >= d && ldt >= d, "%s: the row pitches %lld / %lld do not cover %lld columns", who, (long long)ldx, (long long)ldt, (long long)d);
    const int64_t es = (int64_t)dtype_size(dtype);
    const int vec = d % 8 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)table % 16 == 0 && (ldx * es) % 16 == 0 && (ldt * es) % 16 == 0;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((lm_head_ce_target_logit_kernel<E>), dim3(grid_cap(M, LH_ROWS, LH_GRID_CAP)), dim3(LH_THREADS), 0, stream, (const E*)x, ldx,
                           (const E*)table, ldt, targets, zt, M, (int)V, (int)d, vec);
        return iseg_check_launch(who);
    });
}

extern "C" int iseg_lm_head_ce_finalise(const float* m, const float* s, const float* zt, const int32_t* argmax, const int32_t* targets,
                                        const float* weights, float* loss, float* lse, int32_t* match, float* sums, void* scratch,
                                        size_t scratch_bytes, int64_t M, int64_t V, float scale, hipStream_t stream) {
    const char* who = "iseg_lm_head_ce_finalise";
    ISEG_REQUIRE(m && s && zt && argmax && targets && loss && lse && match && sums && M > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(V >= 1 && V <= INT_MAX, "%s: the vocabulary is 1 .. 2^31 - 1 entries, got %lld", who, (long long)V);
    ISEG_REQUIRE(fin_blocks(M) <= INT_MAX, "%s: too many rows", who);
    ISEG_NEED_WORKSPACE(who, scratch, scratch_bytes, iseg_lm_head_ce_scratch_bytes(M));
    ISEG_REQUIRE((uintptr_t)scratch % 4 == 0, "%s: the scratch buffer must be 4-byte aligned", who);
    float* partials = (float*)scratch;
    hipLaunchKernelGGL(lm_head_ce_finalise_kernel, dim3((unsigned)fin_blocks(M)), dim3(LH_FIN_ROWS), 0, stream, m, s, zt, argmax, targets, weights, loss,
                       lse, match, partials, M, (int)V, scale);
    hipLaunchKernelGGL(lm_head_ce_sums_kernel, dim3(1), dim3(256), 0, stream, (const float*)partials, fin_blocks(M), sums);
    return iseg_check_launch(who);
}

extern "C" int iseg_lm_head_ce_chunk_bwd(const float* z, int64_t ld, const float* m, const float* s, const int32_t* targets, const float* weights,
                                         const float* upstream, float scale, void* g, int64_t ldg, int64_t M, int64_t V, int64_t v0, int64_t w,
                                         int dtype, hipStream_t stream) {
    const char* who = "iseg_lm_head_ce_chunk_bwd";
    ISEG_REQUIRE(z && m && s && targets && g && M > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(V >= 1 && V <= INT_MAX, "%s: the vocabulary is 1 .. 2^31 - 1 entries, got %lld", who, (long long)V);
    ISEG_REQUIRE(w >= 1 && v0 >= 0 && v0 + w <= V, "%s: the chunk [%lld, %lld) is empty or leaves the vocabulary of %lld", who, (long long)v0,
                 (long long)(v0 + w), (long long)V);
    ISEG_REQUIRE(w <= INT_MAX - 64 * 8, "%s: the chunk is too wide", who);
    ISEG_REQUIRE(ld >= w && ldg >= w, "%s: the row pitches %lld / %lld do not cover %lld columns", who, (long long)ld, (long long)ldg, (long long)w);
    const int vec = (uintptr_t)z % 16 == 0 && ld % 4 == 0 && (uintptr_t)g % 16 == 0 && (ldg * (int64_t)dtype_size(dtype)) % 16 == 0;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((lm_head_ce_chunk_bwd_kernel<E>), dim3(grid_cap(M, LH_ROWS, LH_GRID_CAP)), dim3(LH_THREADS), 0, stream, z, ld, m, s, targets,
                           weights, upstream, scale, (E*)g, ldg, M, (int)V, (int)v0, (int)w, vec);
        return iseg_check_launch(who);
    });
}
