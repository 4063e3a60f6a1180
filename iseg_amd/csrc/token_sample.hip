// Token sampling for GemmaCausalLM.generate (keras_nlp.samplers RandomSampler / TopKSampler / TopPSampler behind nlp/gemma/gemma_causal.py's
// compile(sampler=)): one token id per row of a [B, V] logits matrix from one caller-supplied uniform u per row.  No random numbers are made here.
//
// Total order of a row: value descending, then index ascending; NaN above +inf above the finite values above -inf; -0 ties with +0.  Every
// element gets a monotone integer key of its STORED value (16 bits for bf16, 32 for fp32; all NaNs share the top key), so ties are exactly the
// input's.  If the top of the order is not finite its index is the token (torch.argmax's answer), u is not read.  Otherwise, with
// w_i = exp((x_i - max) / T) and W = sum w: the kept set is everything (RANDOM), the first min(k, V) of the order (TOP_K), or the positions j
// of the first k' whose preceding mass is <= p W (TOP_P: a prefix of the order too); the token is the smallest kept id whose cumulative kept
// weight IN TOKEN-ID ORDER exceeds u S.
//   pass 1  one workgroup per (row, chunk of whole 2048-element tiles): the chunk's top key and its lowest index, then, relative to the chunk's
//           own maximum, the sum of the weights and (TOP_K / TOP_P) a 256-bin histogram of counts and of mass over the top key digit.  Mass is
//           summed as 2^-43 fixed-point integers (LDS integer atomics): the sum does not depend on the order of the additions.
//   pass 2  one workgroup of sixteen wavefronts per row merges the partials in chunk order (each scaled by exp((m_s - M) / T), as the decode
//           merge), walks the histogram from the top to the digit that holds the cut (one wavefront, four buckets to a lane), resolves the
//           remaining key digits with one filtered histogram sweep of the row each, and ends with the cut key tau and the number r of the
//           elements equal to tau that are kept (lowest index first).  Then the draw: every wavefront owns a contiguous range of ids in steps
//           of 2048 (a lane: 32 consecutive ids, four 128-bit loads in flight); if only some of tau's ties are kept the wavefronts count their
//           ties first; each sums its kept weight step by step (wave scans, fixed order) and records the step totals; the wavefront and the
//           step that hold u S follow from the totals, and that one step is summed once more down to the lane and the id.
// No atomics across workgroups, fixed order everywhere else: a second call returns the same tokens.
#include "common.h"
#include "iseg_hip.h"
#include "order_keys.h"

#include <float.h>
#include <limits.h>
#include <math.h>

namespace {

constexpr int TS_TILE = 2048;            // elements per pass-1 tile: 256 threads x 8
constexpr int TS_P1_THREADS = 256;
constexpr int TS_P2_THREADS = 1024;
constexpr int TS_P2_WAVES = TS_P2_THREADS / 64;
constexpr int TS_VPL = 4;                // 8-element vectors a lane loads before it works on them
constexpr int TS_STEP = 64 * TS_VPL * 8;    // elements per wave step of the draw: 64 lanes x 32 consecutive ids
constexpr int64_t TS_VMAX = 1 << 20;
constexpr int TS_MAX_SPLITS = (int)(TS_VMAX / TS_TILE);      // 512
constexpr size_t TS_HEAD_BYTES = 16;                          // u32 top key | u32 its lowest index | u64 fixed-point weight sum
constexpr size_t TS_HIST_BYTES = 256 * 4 + 256 * 8;           // u32 counts | u64 fixed-point mass
constexpr float TS_FIX = 8796093022208.f;                     // 2^43: V <= 2^20 weights <= 1 stay below 2^63

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

// w = exp((x - m) / T) as exp2((x - m) c), c = log2(e) / T rounded once on the host: x - m is exact or rounded once, the product once, so the
// exponent t is off by at most 3 * 2^-24 t and, with v_exp_f32's one ulp, a weight by (3 t e^-t + 2) 2^-24 <= 3.2 * 2^-24 of the largest.  Over
// a row the mass moves by at most (3 mean(t) + 2) 2^-24, mean(t) weighted by mass, and that mean cannot pass ln 2^20 = 13.9 (a weight e^-t
// needs e^t entries to matter): 2.6e-6, inside the 1e-5 of mass the tests allow.  -inf weighs 0; results below 2^-126 flush to 0.
__device__ __forceinline__ float weight_of(float x, float m, float c) { return __builtin_amdgcn_exp2f((x - m) * c); }
__device__ __forceinline__ u64 to_fixed(float w) { return (u64)(w * TS_FIX); }

// blockIdx.x = row * splits + split.  Partial: head (top key, its lowest index, fixed-point weight sum relative to the chunk's own maximum),
// then with `hist` the count and mass histograms over the top key digit.
template <class T>
__global__ __launch_bounds__(TS_P1_THREADS) void token_sample_partial_kernel(const T* __restrict__ logits, int64_t ld, unsigned char* __restrict__ part,
                                                                             size_t pstride, int V, int splits, int tiles, float cexp, int hist,
                                                                             int vec) {
    constexpr int KB = KeyBits<T>::value;
    __shared__ u64 red[TS_P1_THREADS / 64];
    __shared__ uint32_t cnt[256];
    __shared__ u64 mass[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t rowi = blockIdx.x / splits;
    const int split = (int)(blockIdx.x % splits);
    const T* row = logits + rowi * ld;
    const int t0 = (int)((int64_t)split * tiles / splits), t1 = (int)((int64_t)(split + 1) * tiles / splits);
    const int begin = t0 * TS_TILE, end = t1 * TS_TILE < V ? t1 * TS_TILE : V;

    cnt[tid] = 0;
    mass[tid] = 0;
    float x[TS_VPL][8];
    int n[TS_VPL];
    u64 best = 0;      // every key of an element is > 0
    for (int i0 = begin + tid * 8; i0 < end; i0 += TS_VPL * TS_TILE) {      // TS_VPL tiles' loads in flight
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v) n[v] = load8(row, i0 + v * TS_TILE, end, vec, x[v]);
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < n[v]) {
                    const u64 pk = pack_top(key_of<KB>(x[v][j]), i0 + v * TS_TILE + j);
                    best = pk > best ? pk : best;
                }
    }
    best = wave_max_u64(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TS_P1_THREADS / 64; ++w) best = red[w] > best ? red[w] : best;
    const uint32_t topkey = (uint32_t)(best >> 32);
    const bool finite = key_finite<KB>(topkey);
    const float m = finite ? value_of<KB>(topkey) : 0.f;
    __syncthreads();

    u64 lsum = 0;
    for (int i0 = begin + tid * 8; i0 < end; i0 += TS_VPL * TS_TILE) {
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v) n[v] = load8(row, i0 + v * TS_TILE, end, vec, x[v]);
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < n[v]) {
                    const u64 fx = finite ? to_fixed(weight_of(x[v][j], m, cexp)) : 0;
                    lsum += fx;
                    if (hist) {
                        const uint32_t d = key_of<KB>(x[v][j]) >> (KB - 8);
                        atomicAdd(&cnt[d], 1u);
                        if (fx) atomicAdd(&mass[d], fx);
                    }
                }
    }
    lsum = wave_sum_u64(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    unsigned char* p = part + (size_t)blockIdx.x * pstride;
    if (tid == 0) {
        u64 total = 0;
#pragma unroll
        for (int w = 0; w < TS_P1_THREADS / 64; ++w) total += red[w];
        reinterpret_cast<uint32_t*>(p)[0] = topkey;
        reinterpret_cast<uint32_t*>(p)[1] = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFu);
        reinterpret_cast<u64*>(p)[1] = total;
    }
    if (hist) {
        reinterpret_cast<uint32_t*>(p + TS_HEAD_BYTES)[tid] = cnt[tid];
        reinterpret_cast<u64*>(p + TS_HEAD_BYTES + 256 * 4)[tid] = mass[tid];
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One wavefront walks the 256 buckets of a digit from the top, four buckets to a lane: the first bucket that reaches the count limit kq, or
// whose mass carries the preceding mass past pW, holds the cut; cgt / Mgt (the same in every lane) advance over the buckets above it.  If
// rounding between the levels leaves no such bucket the cut is at the end of the last bucket that holds an element.
__device__ int walk_digit(const uint32_t* cnt, const double* mass, int kq, double pW, int lane, int& cgt, double& Mgt) {
    int c[4], lc = 0;
    double m[4], lm = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[i] = (int)cnt[255 - (4 * lane + i)];
        m[i] = mass[255 - (4 * lane + i)];
        lc += c[i];
        lm += m[i];
    }
    int ec = cgt + wave_incl_scan(lc, lane) - lc;
    double em = Mgt + (wave_incl_scan(lm, lane) - lm);
    int stop = -1, stop_c = 0, last = -1, last_c = 0;
    double stop_m = 0.0, last_m = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (c[i]) {
            if (stop < 0 && (ec + c[i] >= kq || em + m[i] > pW)) stop = 255 - (4 * lane + i), stop_c = ec, stop_m = em;
            last = 255 - (4 * lane + i), last_c = ec, last_m = em;
        }
        ec += c[i];
        em += m[i];
    }
    const u64 bs = __ballot(stop >= 0), bl = __ballot(last >= 0);
    if (bs) {
        const int src = __ffsll((long long)bs) - 1;
        cgt = __shfl(stop_c, src);
        Mgt = __shfl(stop_m, src);
        return __shfl(stop, src);
    }
    if (!bl) return 0;
    const int src = 63 - __clzll((long long)bl);
    cgt = __shfl(last_c, src);
    Mgt = __shfl(last_m, src);
    return __shfl(last, src);
}

// blockIdx.x = row
template <class T>
__global__ __launch_bounds__(TS_P2_THREADS) void token_sample_draw_kernel(const T* __restrict__ logits, int64_t ld, const float* __restrict__ u,
                                                                          int32_t* __restrict__ tokens, const unsigned char* __restrict__ part,
                                                                          size_t pstride, int V, int splits, int mode, int kq, float p, float cexp,
                                                                          int vec) {
    constexpr int KB = KeyBits<T>::value;
    constexpr int LEVELS = KB / 8;
    constexpr int MAX_STEPS = (int)(TS_VMAX / TS_STEP);
    __shared__ float sc[TS_MAX_SPLITS];
    __shared__ double term[TS_MAX_SPLITS];
    __shared__ uint32_t cntq[4][256];
    __shared__ double massq[4][256];
    __shared__ uint32_t cnt[256];
    __shared__ u64 massi[256];
    __shared__ double massd[256];
    __shared__ double stepsum[MAX_STEPS];
    __shared__ int stepeq[MAX_STEPS];
    __shared__ u64 red64[TS_P2_WAVES];
    __shared__ double redd[TS_P2_WAVES];
    __shared__ int redi[TS_P2_WAVES];
    __shared__ uint32_t s_prefix;
    __shared__ float s_vtau;
    __shared__ int s_r, s_ranked;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t rowi = blockIdx.x;
    const T* row = logits + rowi * ld;
    const unsigned char* prow = part + (size_t)rowi * splits * pstride;
    const bool hist = mode != ISEG_SAMPLE_RANDOM;

    // ---- the top of the order over the chunks (splits <= 512: a thread reads at most one head) ----
    u64 best = 0, lfix = 0;
    uint32_t mk = 0;
    if (tid < splits) {
        const unsigned char* h = prow + (size_t)tid * pstride;
        mk = reinterpret_cast<const uint32_t*>(h)[0];
        best = pack_top(mk, (int)reinterpret_cast<const uint32_t*>(h)[1]);
        lfix = reinterpret_cast<const u64*>(h)[1];
    }
    best = wave_max_u64(best);
    if (lane == 0) red64[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TS_P2_WAVES; ++w) best = red64[w] > best ? red64[w] : best;
    const uint32_t topkey = (uint32_t)(best >> 32);
    const int topidx = (int)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFu));
    if (!key_finite<KB>(topkey)) {      // NaN, +inf or an all -inf row: torch.argmax's answer, u is not read
        if (tid == 0) tokens[rowi] = topidx;
        return;
    }
    const float M = value_of<KB>(topkey);

    // ---- merge in chunk order: every chunk's sums were taken relative to its own maximum ----
    if (tid < splits) {
        const float f = key_finite<KB>(mk) ? weight_of(value_of<KB>(mk), M, cexp) : 0.f;
        sc[tid] = f;
        term[tid] = (double)f * (double)lfix;
    }
    __syncthreads();
    if (hist) {      // a quarter of the chunks to each 256 threads, eight loads in flight, added in chunk order
        const int q = tid >> 8, d = tid & 255;
        const int sb = (int)((int64_t)q * splits / 4), se = (int)((int64_t)(q + 1) * splits / 4);
        uint32_t c = 0;
        double ms = 0.0;
        for (int s0 = sb; s0 < se; s0 += 8) {
            uint32_t cc[8];
            u64 mm[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned char* h = prow + (size_t)(s0 + k < se ? s0 + k : sb) * pstride + TS_HEAD_BYTES;
                cc[k] = reinterpret_cast<const uint32_t*>(h)[d];
                mm[k] = reinterpret_cast<const u64*>(h + 256 * 4)[d];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (s0 + k < se) {
                    c += cc[k];
                    ms += (double)sc[s0 + k] * (double)mm[k];
                }
        }
        cntq[q][d] = c;
        massq[q][d] = ms;
        __syncthreads();
        if (tid < 256) {
            cnt[tid] = cntq[0][tid] + cntq[1][tid] + cntq[2][tid] + cntq[3][tid];
            massd[tid] = ((massq[0][tid] + massq[1][tid]) + massq[2][tid]) + massq[3][tid];
        }
        __syncthreads();
    }

    // ---- the cut key tau and the number r of its ties that are kept (masses in units of 2^-43); wavefront 0 decides ----
    int cgt = 0;
    double Mgt = 0.0, pW = INFINITY;
    if (hist) {
        if (wave == 0) {
            if (mode == ISEG_SAMPLE_TOP_P) {
                double W = 0.0;
                for (int s = lane; s < splits; s += 64) W += term[s];
                pW = (double)p * wave_sum_f64(W);
            }
            const int d = walk_digit(cnt, massd, kq, pW, lane, cgt, Mgt);
            if (lane == 0) s_prefix = (uint32_t)d;
        }
        for (int level = 1; level < LEVELS; ++level) {
            __syncthreads();
            const uint32_t prefix = s_prefix;
            if (tid < 256) cnt[tid] = 0, massi[tid] = 0;
            __syncthreads();
            const int above = KB - 8 * level;      // key bits below the resolved prefix
            // the values whose keys carry the prefix, as a float range: a cheap filter in front of the key
            const uint32_t klo = prefix << above, khi = klo | ((1u << above) - 1u), kmin = key_of<KB>(-INFINITY), kmax = key_of<KB>(INFINITY);
            const float lo = value_of<KB>(klo < kmin ? kmin : klo), hi = value_of<KB>(khi > kmax ? kmax : khi);
            float x[TS_VPL][8];
            int n[TS_VPL];
            for (int i0 = tid * 8; i0 < V; i0 += TS_VPL * TS_P2_THREADS * 8) {      // TS_VPL loads in flight per thread
#pragma unroll
                for (int v = 0; v < TS_VPL; ++v) n[v] = load8(row, i0 + v * TS_P2_THREADS * 8, V, vec, x[v]);
#pragma unroll
                for (int v = 0; v < TS_VPL; ++v)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (j < n[v] && x[v][j] >= lo && x[v][j] <= hi) {
                            const uint32_t key = key_of<KB>(x[v][j]);
                            if ((key >> above) == prefix) {      // (+0 and -0 share a key but lie in the ranges of two prefixes)
                                const uint32_t d = (key >> (above - 8)) & 255u;
                                atomicAdd(&cnt[d], 1u);
                                const u64 fx = to_fixed(weight_of(x[v][j], M, cexp));
                                if (fx) atomicAdd(&massi[d], fx);
                            }
                        }
            }
            __syncthreads();
            if (tid < 256) massd[tid] = (double)massi[tid];
            __syncthreads();
            if (wave == 0) {
                const int d = walk_digit(cnt, massd, kq, pW, lane, cgt, Mgt);
                if (lane == 0) s_prefix = (prefix << 8) | (uint32_t)d;
            }
        }
        if (tid == 0) {
            const uint32_t tau = s_prefix;
            const int ctau = (int)cnt[tau & 255u];
            int r = kq - cgt < ctau ? kq - cgt : ctau;
            if (mode == ISEG_SAMPLE_TOP_P) {      // tie t of tau is kept iff Mgt + t w <= pW
                const double wt = (double)weight_of(value_of<KB>(tau), M, cexp) * (double)TS_FIX;
                if (wt > 0.0) {
                    const double room = pW - Mgt;
                    const double tp = room < 0.0 ? 0.0 : floor(room / wt) + 1.0;
                    if (tp < (double)r) r = (int)tp;
                }
                if (cgt == 0 && r < 1) r = 1;      // the first of the order is always kept
            }
            s_vtau = value_of<KB>(tau);
            s_r = r;
            s_ranked = r > 0 && r < ctau;      // only then does a tie's rank among the ties matter
        }
    } else if (tid == 0) {
        s_vtau = -INFINITY;      // everything is kept (-inf entries as ties of weight 0)
        s_r = 1;
        s_ranked = 0;
    }
    __syncthreads();
    // kept: x > vtau, or x == vtau and the tie's rank among the ties (by index) is below r.  Values compare as their keys do: the top is
    // finite, so no NaN is left, and -0 == +0 on both sides
    const float vtau = s_vtau;
    const int r = s_r;
    const bool ranked = s_ranked != 0;
    const bool all_ties = !ranked && r > 0;

    // ---- the draw: wavefront w owns the ids of the steps [w * steps / 16, (w + 1) * steps / 16); in a step a lane owns 32 consecutive ids ----
    const int steps = (V + TS_STEP - 1) / TS_STEP;
    const int st0 = (int)((int64_t)wave * steps / TS_P2_WAVES), st1 = (int)((int64_t)(wave + 1) * steps / TS_P2_WAVES);
    float x[TS_VPL][8];
    int n[TS_VPL];
    auto load_step = [&](int st) {
        const int i0 = st * TS_STEP + lane * (TS_VPL * 8);
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v) n[v] = load8(row, i0 + v * 8, V, vec, x[v]);
    };
    auto count_ties = [&]() {
        int ce = 0;
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j) ce += (j < n[v] && x[v][j] == vtau) ? 1 : 0;
        return ce;
    };
    int eq0 = 0;      // ties of tau at ids below this wavefront's range
    if (ranked) {
        int ce = 0;
        for (int st = st0; st < st1; ++st) {
            load_step(st);
            ce += count_ties();
        }
        ce = wave_incl_scan(ce, lane);
        if (lane == 63) redi[wave] = ce;
        __syncthreads();
        for (int w = 0; w < wave; ++w) eq0 += redi[w];
    }

    // the kept weight of one step in id order: fp32 sums of eight, fp64 from there on, then an inclusive wave scan; `eqbase` counts the ties
    // of the wavefront's range in front of the step
    auto step_sum = [&](int st, int& eqbase, double& excl, int& lane_eq) -> double {
        load_step(st);
        if (ranked) {
            const int ce = count_ties();
            const int inc = wave_incl_scan(ce, lane);
            lane_eq = eqbase + inc - ce;
            eqbase += __shfl(inc, 63);
        }
        double ls = 0.0;
        int e = lane_eq;
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v) {
            float fs = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < n[v]) {
                    const float xv = x[v][j];
                    const bool keep = xv > vtau || (xv == vtau && (ranked ? e++ < r : all_ties));
                    fs += keep ? weight_of(xv, M, cexp) : 0.f;
                }
            ls += (double)fs;
        }
        const double inc = wave_incl_scan(ls, lane);
        excl = inc - ls;
        return inc;
    };

    double run = 0.0, excl;
    int eqbase = eq0, lane_eq = 0;
    for (int st = st0; st < st1; ++st) {
        if (lane == 0) stepeq[st] = eqbase;
        const double tot = __shfl(step_sum(st, eqbase, excl, lane_eq), 63);
        if (lane == 0) stepsum[st] = tot;
        run += tot;
    }
    if (lane == 0) redd[wave] = run;
    __syncthreads();
    double before = 0.0, S = 0.0;      // kept weight below this wavefront's range; of the row
    int target_wave = TS_P2_WAVES - 1;
    float ur = u[rowi];
    ur = ur >= 0.f ? (ur < 1.f ? ur : 1.f) : 0.f;
    for (int w = 0; w < TS_P2_WAVES; ++w) {
        if (w == wave) before = S;
        S += redd[w];
    }
    double target = (double)ur * S;
    const double below = S * (1.0 - 1.1102230246251565e-16);      // rounding left nothing above u S: the last id that raised the sum
    target = target < below ? target : below;
    {
        double c = 0.0;
        for (int w = 0; w < TS_P2_WAVES; ++w) {
            c += redd[w];
            if (c > target) {
                target_wave = w;
                break;
            }
        }
    }
    if (wave != target_wave || st0 >= st1) {
        if (wave == target_wave && lane == 0) tokens[rowi] = topidx;      // not reached: a wavefront without a step has no weight
        return;
    }

    // the step that holds u S from the recorded totals (the same running sum), then that step's sums once more down to the id
    int st = st0;
    run = 0.0;
    for (; st < st1 - 1; ++st) {
        const double t = stepsum[st];
        if (before + (run + t) > target) break;
        run += t;
    }
    eqbase = stepeq[st];
    const double inc = step_sum(st, eqbase, excl, lane_eq);
    const u64 b = __ballot(before + (run + inc) > target);
    const int first = b ? __ffsll((long long)b) - 1 : 63;
    int found = -1, lastpos = -1;      // lastpos: the highest id of this lane that is kept with a weight > 0
    if (lane <= first) {
        double c = 0.0;
        int e = lane_eq;
#pragma unroll
        for (int v = 0; v < TS_VPL; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < n[v]) {
                    const float xv = x[v][j];
                    const bool keep = xv > vtau || (xv == vtau && (ranked ? e++ < r : all_ties));
                    const float w = keep ? weight_of(xv, M, cexp) : 0.f;
                    if (w > 0.f) {
                        c += (double)w;
                        lastpos = st * TS_STEP + lane * (TS_VPL * 8) + v * 8 + j;
                        if (found < 0 && lane == first && before + (run + (excl + c)) > target) found = lastpos;
                    }
                }
    }
    // the scan and the walk round differently: if the walk did not cross, the last id at or below the lane that carried weight
    int tok = lane <= first ? lastpos : -1;
    const int crossed = __shfl(found, first);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const int o = __shfl_xor(tok, off);
        tok = o > tok ? o : tok;
    }
    if (lane == 0) tokens[rowi] = crossed >= 0 ? crossed : tok >= 0 ? tok : topidx;
}

int ts_tiles(int64_t V) { return (int)ceil_div64(V, TS_TILE); }

// chunks of the launcher's own plan: enough workgroups for two per CU of a 256-CU chip, at least two tiles per chunk
int ts_plan(int64_t batch, int64_t V) {
    const int64_t want = ceil_div64(512, batch < 1 ? 1 : batch), most = ts_tiles(V) / 2;
    return (int)(want < most ? want : most < 1 ? 1 : most);
}

int ts_resolve(int64_t batch, int64_t V, int splits) {
    if (splits <= 0) return ts_plan(batch, V);
    const int tiles = ts_tiles(V);
    return splits < tiles ? splits : tiles;
}

size_t ts_partial_bytes(int mode) { return TS_HEAD_BYTES + (mode == ISEG_SAMPLE_RANDOM ? 0 : TS_HIST_BYTES); }

}  // namespace

#define TS_UNSUPPORTED(cond, ...)             \
    do {                                      \
        if (!(cond)) {                        \
            iseg_set_error(__VA_ARGS__);      \
            return ISEG_ERR_UNSUPPORTED;      \
        }                                     \
    } while (0)

extern "C" int iseg_token_sample_supported(int64_t V, int mode, int k, int dtype) {
    const bool mode_ok = mode == ISEG_SAMPLE_RANDOM || mode == ISEG_SAMPLE_TOP_K || mode == ISEG_SAMPLE_TOP_P;
    return ((dtype == ISEG_BF16 || dtype == ISEG_F32) && V >= 1 && V <= TS_VMAX && mode_ok && k >= 0 && (mode != ISEG_SAMPLE_TOP_K || k >= 1)) ? 1 : 0;
}

extern "C" int iseg_token_sample_splits(int64_t batch, int64_t V) {
    if (batch < 1 || V < 1 || V > TS_VMAX) return 0;
    return ts_plan(batch, V);
}

extern "C" size_t iseg_token_sample_scratch_bytes(int64_t batch, int64_t V, int mode, int k, int splits) {
    if (batch < 1 || !iseg_token_sample_supported(V, mode, k, ISEG_F32)) return 0;
    return (size_t)batch * ts_resolve(batch, V, splits) * ts_partial_bytes(mode);
}

extern "C" int iseg_token_sample(const void* logits, int64_t ld, const float* u, int32_t* tokens, void* ws, size_t ws_bytes, int64_t batch, int64_t V,
                                 int mode, int k, float p, float temperature, int splits, int dtype, hipStream_t stream) {
    const char* who = "iseg_token_sample";
    ISEG_REQUIRE(logits && u && tokens && batch > 0, "%s: bad arguments", who);
    TS_UNSUPPORTED(iseg_token_sample_supported(V, mode, k, dtype),
                   "%s: needs bf16 or fp32 logits, 1 <= V <= 2^20, a mode of ISEG_SAMPLE_*, k >= 0 and k >= 1 for top-k (got V %lld, mode %d, k %d, dtype %d)",
                   who, (long long)V, mode, k, dtype);
    ISEG_REQUIRE(temperature > 0.f && temperature <= FLT_MAX && 1.4426950408889634f / temperature <= FLT_MAX,
                 "%s: needs a positive finite temperature (with a finite 1 / temperature), got %g", who, (double)temperature);
    ISEG_REQUIRE(p > 0.f && p <= 1.f, "%s: p must lie in (0, 1], got %g", who, (double)p);
    ISEG_REQUIRE(ld >= V, "%s: the row pitch %lld does not cover %lld columns", who, (long long)ld, (long long)V);
    const int nsplit = ts_resolve(batch, V, splits), tiles = ts_tiles(V);
    ISEG_REQUIRE(batch * nsplit <= INT_MAX, "%s: too many work items", who);
    ISEG_NEED_WORKSPACE(who, ws, ws_bytes, iseg_token_sample_scratch_bytes(batch, V, mode, k, nsplit));
    ISEG_REQUIRE((uintptr_t)ws % 8 == 0, "%s: the scratch buffer must be 8-byte aligned", who);
    const size_t esize = dtype_size(dtype), pstride = ts_partial_bytes(mode);
    const int vec = (uintptr_t)logits % 16 == 0 && (ld * (int64_t)esize) % 16 == 0;
    const int kq = mode == ISEG_SAMPLE_TOP_P && k == 0 ? (int)V : k < V ? k : (int)V;
    const float cexp = 1.4426950408889634f / temperature;
    unsigned char* part = (unsigned char*)ws;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((token_sample_partial_kernel<E>), dim3((unsigned)(batch * nsplit)), dim3(TS_P1_THREADS), 0, stream, (const E*)logits, ld, part,
                           pstride, (int)V, nsplit, tiles, cexp, mode != ISEG_SAMPLE_RANDOM ? 1 : 0, vec);
        hipLaunchKernelGGL((token_sample_draw_kernel<E>), dim3((unsigned)batch), dim3(TS_P2_THREADS), 0, stream, (const E*)logits, ld, u, tokens,
                           (const unsigned char*)part, pstride, (int)V, nsplit, mode, kq, p, cexp, vec);
        return iseg_check_launch(who);
    });
}
