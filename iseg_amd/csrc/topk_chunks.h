// The split-V pass that beam_search.hip and contrastive.hip share: one read of a logits row in chunks of whole 2048-element tiles, per chunk the
// fp64 sum of the softmax weights relative to the chunk's own maximum and the chunk's n first entries of the row order of order_keys.h; the chunk
// plan; and the merge of one row's chunk records (top key, weight sum, the row's n first entries).  beam_search.hip's first lines have the
// derivation of the weight's accuracy.
#pragma once
#include "common.h"
#include "order_keys.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int BS_TILE = 2048;            // elements per tile: 256 threads x 8
constexpr int BS_P1_THREADS = 256;
constexpr int BS_P1_WAVES = BS_P1_THREADS / 64;
constexpr int BS_VPL = 4;                // 8-element vectors (tiles) a thread loads before it works on them
constexpr int BS_MAX_NB = 16;
constexpr int BS_P2_THREADS = BS_MAX_NB * 64;      // a wavefront per beam row
constexpr int64_t BS_VMAX = 1 << 20;

static_assert(BS_P1_WAVES * BS_MAX_NB == 64, "the pass-1 merge gives one wavefront entry to each lane of the first wavefront");

// c is earlier in the order than nothing yet (`first`) or strictly later than `prev`, the entry taken last: the next to take is the largest such
__device__ __forceinline__ bool bs_open(u64 c, u64 prev, bool first) { return first || c < prev; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// exp2((x - m) c), c = log2(e) / T in fp64: the exponent is exact to 2^-53, hi is its fp32 head and lo the rest (|lo| <= 2^-24 |hi|), so
// exp2(hi + lo) = exp2(hi) (1 + lo ln 2) up to (lo ln 2)^2 / 2 < 2^-34 where exp2(hi) is not flushed to 0.  x = -inf weighs 0.
__device__ __forceinline__ float bs_weight(float x, float m, double c) {
    const double e = ((double)x - (double)m) * c;
    const float hi = (float)e;
    const float lo = fabsf(hi) <= FLT_MAX ? (float)(e - (double)hi) : 0.f;
    return __builtin_amdgcn_exp2f(hi) * fmaf(lo, 0.6931471805599453f, 1.f);
}

// blockIdx.x = row * splits + split.  rowmap (or NULL): output row r reads logits row r * group + clamp(rowmap[r], 0, group - 1).  Record of pstride u64: the bits of the fp64 weight sum relative to the chunk's own maximum (the value of
// the first pair's key; 0 unless that is finite), then nb packed (key, index) pairs in the row's order, 0 where the chunk has fewer elements.
template <class T>
__global__ __launch_bounds__(BS_P1_THREADS) void beam_select_partial_kernel(const T* __restrict__ logits, int64_t ld, u64* __restrict__ part, int pstride,
                                                                            int V, int splits, int tiles, int nb, double cexp, int vec,
                                                                            const int32_t* __restrict__ rowmap, int group) {
    constexpr int KB = KeyBits<T>::value;
    __shared__ u64 top[BS_MAX_NB];
    __shared__ u64 wtop[BS_P1_WAVES][BS_MAX_NB];
    __shared__ u64 wmax[BS_P1_WAVES];
    __shared__ double wsum[BS_P1_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t rowi = blockIdx.x / splits;
    if (rowmap) {
        const int w = rowmap[rowi];
        rowi = rowi * group + (w < 0 ? 0 : w >= group ? group - 1 : w);
    }
    const int split = (int)(blockIdx.x % splits);
    const T* row = logits + rowi * ld;
    const int t0 = (int)((int64_t)split * tiles / splits), t1 = (int)((int64_t)(split + 1) * tiles / splits);
    const int begin = t0 * BS_TILE, end = t1 * BS_TILE < V ? t1 * BS_TILE : V;

    if (tid < BS_MAX_NB) top[tid] = 0;
    __syncthreads();
    uint32_t runkey = 0;      // the top key so far (every key of an element is > 0)
    double s = 0.0;           // this thread's weights relative to value_of(runkey)
    float x[BS_VPL][8];
    int n[BS_VPL];
    u64 pk[BS_VPL][8];
    for (int b0 = begin; b0 < end; b0 += BS_VPL * BS_TILE) {      // the same trips for every thread: there are barriers inside
        const int i0 = b0 + tid * 8;
#pragma unroll
        for (int v = 0; v < BS_VPL; ++v) n[v] = load8(row, i0 + v * BS_TILE, end, vec, x[v]);
        u64 lm = 0;
#pragma unroll
        for (int v = 0; v < BS_VPL; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                pk[v][j] = j < n[v] ? pack_top(key_of<KB>(x[v][j]), i0 + v * BS_TILE + j) : 0;
                lm = pk[v][j] > lm ? pk[v][j] : lm;
            }
        const u64 wm = wave_max_u64(lm);
        if (lane == 0) wmax[wave] = wm;
        __syncthreads();
        u64 bm = wmax[0];
#pragma unroll
        for (int w = 1; w < BS_P1_WAVES; ++w) bm = wmax[w] > bm ? wmax[w] : bm;
        const u64 tau = top[nb - 1];      // an entry has to beat the current nb-th to enter the list

        // ---- the running maximum and this thread's share of the weight sum ----
        const uint32_t bkey = (uint32_t)(bm >> 32);
        if (bkey > runkey) {
            s = key_finite<KB>(runkey) && key_finite<KB>(bkey) ? s * exp2(((double)value_of<KB>(runkey) - (double)value_of<KB>(bkey)) * cexp) : 0.0;
            runkey = bkey;
        }
        if (key_finite<KB>(runkey)) {
            const float m = value_of<KB>(runkey);
#pragma unroll
            for (int v = 0; v < BS_VPL; ++v)
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < n[v]) s += (double)bs_weight(x[v][j], m, cexp);
        }

        // ---- this wavefront's entries that beat tau, in order ----
        bool live = wm > tau;
        u64 prev = 0;
        for (int r = 0; r < nb; ++r) {
            u64 res = 0;
            if (live) {
                u64 l = 0;
#pragma unroll
                for (int v = 0; v < BS_VPL; ++v)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const u64 c = pk[v][j];
                        l = (bs_open(c, prev, r == 0) && c > l) ? c : l;
                    }
                res = wave_max_u64(l);
                if (res <= tau) res = 0, live = false;
                prev = res;
            }
            if (lane == 0) wtop[wave][r] = res;
        }
        __syncthreads();
        // ---- the first wavefront merges them with the list (lane l: entry l & 15 of wavefront l >> 4, and entry l of the list) ----
        if (wave == 0 && bm > tau) {
            const u64 c0 = (lane & 15) < nb ? wtop[lane >> 4][lane & 15] : 0;
            const u64 c1 = lane < nb ? top[lane] : 0;
            u64 mine = 0;
            prev = 0;
            for (int r = 0; r < nb; ++r) {
                u64 l = bs_open(c0, prev, r == 0) ? c0 : 0;
                l = (bs_open(c1, prev, r == 0) && c1 > l) ? c1 : l;
                const u64 res = wave_max_u64(l);
                if (lane == r) mine = res;
                prev = res;
                if (res == 0) break;
            }
            if (lane < nb) top[lane] = mine;
        }
        // (no barrier here: the next trip's first one orders these writes in front of every read of `top`, and wmax / wtop are rewritten only
        // after a barrier that their readers reach after reading)
    }
    __syncthreads();
    s = wave_sum_f64(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    u64* p = part + (size_t)blockIdx.x * pstride;
    if (tid == 0) {
        double total = wsum[0];
#pragma unroll
        for (int w = 1; w < BS_P1_WAVES; ++w) total += wsum[w];
        p[0] = (u64)__double_as_longlong(key_finite<KB>(runkey) ? total : 0.0);
    }
    if (tid < nb) p[1 + tid] = top[tid];
}

// One wavefront merges the chunk records of one row (prow: its `splits` records): the row's top key, the fp64 weight sum relative to the value
// of that key (a lane adds its chunks in chunk order, the lanes' sums go through one butterfly; chunks of -inf alone weigh nothing; call it
// only where the top key is finite) and, in lane r < nb, the row's r-th entry over all records (0: the row has fewer).
__device__ __forceinline__ uint32_t bs_row_top(const u64* __restrict__ prow, int pstride, int splits, int lane) {
    u64 best = 0;
    for (int sp = lane; sp < splits; sp += 64) {
        const u64 e = prow[(size_t)sp * pstride + 1];
        best = e > best ? e : best;
    }
    return (uint32_t)(wave_max_u64(best) >> 32);
}

template <int KB> __device__ __forceinline__ double bs_row_sum(const u64* __restrict__ prow, int pstride, int splits, int lane, float M, double cexp) {
    double acc = 0.0;
    for (int sp = lane; sp < splits; sp += 64) {
        const uint32_t mk = (uint32_t)(prow[(size_t)sp * pstride + 1] >> 32);
        if (key_finite<KB>(mk))
            acc += exp2(((double)value_of<KB>(mk) - (double)M) * cexp) * __longlong_as_double((long long)prow[(size_t)sp * pstride]);
    }
    return wave_sum_f64(acc);
}

__device__ __forceinline__ u64 bs_row_entries(const u64* __restrict__ prow, int pstride, int splits, int nb, int lane) {
    u64 prev = 0, entry = 0;
    for (int r = 0; r < nb; ++r) {
        u64 l = 0;
        for (int i = lane; i < splits * nb; i += 64) {
            const u64 c = prow[(size_t)(i / nb) * pstride + 1 + i % nb];
            l = (bs_open(c, prev, r == 0) && c > l) ? c : l;
        }
        const u64 res = wave_max_u64(l);
        if (lane == r) entry = res;
        prev = res;
        if (res == 0) break;
    }
    return entry;
}

int bs_tiles(int64_t V) { return (int)ceil_div64(V, BS_TILE); }

// chunks of the launcher's own plan: enough workgroups for two per CU of a 256-CU chip, at least two tiles per chunk
int bs_plan(int64_t rows, int64_t V) {
    const int64_t want = ceil_div64(512, rows < 1 ? 1 : rows), most = bs_tiles(V) / 2;
    return (int)(want < most ? want : most < 1 ? 1 : most);
}

int bs_resolve(int64_t rows, int64_t V, int splits) {
    if (splits <= 0) return bs_plan(rows, V);
    const int tiles = bs_tiles(V);
    return splits < tiles ? splits : tiles;
}

}  // namespace
