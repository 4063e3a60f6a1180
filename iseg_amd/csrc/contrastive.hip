// One step of keras_nlp.samplers.ContrastiveSampler for GemmaCausalLM.generate: the k most probable tokens of a row with their probabilities
// (iseg_contrastive_candidates), the degeneration penalty and the winner (iseg_contrastive_select) and the winner's hand-over to the other
// k - 1 rows of its group, in place (iseg_contrastive_commit).  Row b * k + j is candidate j of batch row b, the layout of beam_search.hip;
// include/iseg_hip.h has the full statement.
//
// Candidates.  softmax(x / T) is monotone in x, so a row's candidates are its k first entries in the order of order_keys.h, and the pass that
// finds them and the softmax sum is beam_search.hip's (topk_chunks.h: one read of the logits, no [B, V] tensor, fp64 sums in a fixed order);
// an optional row map makes output row b read logits row b * group + map[b], so the previous step's winner is never gathered.  The merge, one
// wavefront per output row, forms p = exp2((x - M) log2(e) / T) / sum in fp64 and rounds once.
//
// Select.  sim[j, t] = <h_t, c_j> / (|h_t| |c_j|) for t < index, max over t, score = (1 - alpha) p - alpha max sim, argmax.  Vector dot products,
// not the matrix cores: with k <= 16 rows an MFMA tile would be mostly padding, and the k D FMAs per position (5 * 2048 at Gemma-2B) stay below
// the time the position's D elements take to arrive from memory; plain fp32 FMAs in a fixed order also make every sim the same bits whichever
// workgroup computes it.  |h_t|^2 is recomputed from the loaded elements (one more FMA per element, 1 / k of the work): no side buffer that the
// commit would have to keep in step.
//   pass 1  blockIdx = ((b, split), candidate group).  The group's candidates (all k where k D elements fit 128 KB of LDS) are copied to LDS as
//           stored; their squared norms, one wavefront per candidate.  Each wavefront then takes 4 positions of the split at a time: a lane
//           loads 8 consecutive elements of each position per 512-element trip over D, adds their squares and, per candidate, the 8 products
//           with the candidate's elements from LDS; 64-lane butterflies; lane j forms sim[j, t] and keeps the largest key (order_keys.h: NaN
//           on top, so a NaN similarity wins the maximum as torch.max has it).  The four wavefronts' keys meet in LDS: one u32 per (split, j).
//   pass 2  one wavefront per batch row: lane j takes the maximum over the splits, forms the score, and the first maximal score wins.
// A position's arithmetic does not depend on the split it falls into, and a maximum of keys does not depend on the grouping: the outputs are
// bit-identical for every `splits`.  Positions >= index are never read.  No atomics.
//
// Commit.  Per group, 16-byte columns: the winner's cache row at the step's position on every plane goes to the other rows of the group, its
// token likewise, its hidden state into the history.  Nothing else is touched; a thread reads the winner's column and writes the others'.
#include "common.h"
#include "iseg_hip.h"
#include "order_keys.h"
#include "topk_chunks.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int CS_MAX_K = BS_MAX_NB;
constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_P = 4;                          // positions a wavefront works on at a time
constexpr int CS_TRIP = 64 * 8;                  // elements of D per trip: 8 per lane
constexpr int64_t CS_LDS_MAX = 128 * 1024;       // candidates resident in LDS per workgroup
constexpr int64_t CS_DMAX = 16384;
constexpr int64_t CS_GRID_CAP = 16384;

typedef __attribute__((ext_vector_type(4))) unsigned int cs_u32x4;

// ---------------------------------------------------------------- candidates ----------------------------------------------------------------
// blockIdx.x = output row; one wavefront
template <class T>
__global__ __launch_bounds__(64) void contrastive_candidates_merge_kernel(float* __restrict__ probs, int32_t* __restrict__ tokens, const u64* __restrict__ part,
                                                                          int pstride, int splits, int k, double cexp) {
    constexpr int KB = KeyBits<T>::value;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const u64* prow = part + (size_t)b * splits * pstride;
    const uint32_t topkey = bs_row_top(prow, pstride, splits, lane);
    if (!key_finite<KB>(topkey)) {      // NaN, +inf, or -inf alone on top: the softmax is NaN throughout, every token ties: the first k ids
        if (lane < k) probs[b * k + lane] = NAN, tokens[b * k + lane] = lane;
        return;
    }
    const float M = value_of<KB>(topkey);
    const double sum = bs_row_sum<KB>(prow, pstride, splits, lane, M, cexp);
    const u64 entry = bs_row_entries(prow, pstride, splits, k, lane);
    if (lane < k) {
        float p = NAN;
        int idx = lane;      // not reached: k <= V gives every lane < k an entry
        if (entry) {
            const float xv = value_of<KB>((uint32_t)(entry >> 32));
            idx = (int)(0xFFFFFFFFu - (uint32_t)(entry & 0xFFFFFFFFu));
            p = (float)(exp2(((double)xv - (double)M) * cexp) / sum);
        }
        probs[b * k + lane] = p;
        tokens[b * k + lane] = idx;
    }
}

// ------------------------------------------------------------------ select ------------------------------------------------------------------
struct CsPlan {
    int kc;       // candidates per workgroup
    int ncg;      // candidate groups
    size_t lds;   // bytes of LDS for kc candidates
};

CsPlan cs_plan(int64_t D, int k, int dtype) {
    const int64_t row = D * (int64_t)dtype_size(dtype);
    int64_t cap = CS_LDS_MAX / row;
    cap = cap < 1 ? 1 : cap;
    const int ncg = (int)ceil_div64(k, cap);
    const int kc = (int)ceil_div64(k, ncg);
    return {kc, (int)ceil_div64(k, kc), (size_t)(kc * row)};
}

// enough workgroups for two per CU of a 256-CU chip, at least 16 positions (4 per wavefront) each
int cs_splits(int64_t groups, int64_t index, int ncg) {
    const int64_t wgs = (groups < 1 ? 1 : groups) * ncg, want = ceil_div64(512, wgs), most = index / 16;
    return (int)(want < most ? want : most < 1 ? 1 : most);
}

int cs_resolve(int64_t groups, int64_t index, int ncg, int splits) {
    if (splits <= 0) return cs_splits(groups, index, ncg);
    return (int)(splits < index ? splits : index);
}

template <class T> __device__ __forceinline__ void cs_copy8(T* dst, const T* src) {
    const cs_u32x4* s = reinterpret_cast<const cs_u32x4*>(src);
    cs_u32x4* d = reinterpret_cast<cs_u32x4*>(dst);
#pragma unroll
    for (int i = 0; i < (int)(8 * sizeof(T) / 16); ++i) d[i] = s[i];
}

// blockIdx.x = (b * splits + split) * ncg + candidate group.  part[(b * splits + split) * k + j]: the largest key of sim[j, t] over the split
template <class T, int KC>
__global__ __launch_bounds__(CS_THREADS) void contrastive_sim_kernel(const T* __restrict__ hist, int64_t hs_b, int64_t hs_t, const T* __restrict__ cand,
                                                                     int64_t ldc, uint32_t* __restrict__ part, int index, int D, int k, int kc, int ncg,
                                                                     int splits) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
    __shared__ float cnorm2[CS_MAX_K];
    __shared__ uint32_t wbest[CS_WAVES][CS_MAX_K];
    T* cl = reinterpret_cast<T*>(cs_lds);      // [nk][D]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = (int)(blockIdx.x % ncg);
    const int64_t bs = blockIdx.x / ncg, b = bs / splits;
    const int split = (int)(bs % splits);
    const int j0 = cg * kc, nk = k - j0 < kc ? k - j0 : kc;

    const T* crow = cand + (b * k + j0) * ldc;
    for (int i = tid * 8; i < nk * D; i += CS_THREADS * 8) cs_copy8(cl + i, crow + (int64_t)(i / D) * ldc + i % D);
    __syncthreads();
    for (int j = wave; j < nk; j += CS_WAVES) {
        float s = 0.f, c[8];
        for (int d0 = lane * 8; d0 < D; d0 += CS_TRIP) {
            ::load8(cl + j * D + d0, c);
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(c[e], c[e], s);
        }
        s = wave_sum(s);
        if (lane == 0) cnorm2[j] = s;
    }
    __syncthreads();

    const int t0 = (int)((int64_t)split * index / splits), t1 = (int)((int64_t)(split + 1) * index / splits);
    const T* hb = hist + b * hs_b;
    const float cn = lane < nk ? sqrtf(cnorm2[lane]) : 0.f;
    uint32_t best = 0;      // lane j: the largest key of sim[j0 + j, t] over this wavefront's positions (every key of a number or a NaN is > 0)
    for (int tb = t0 + wave * CS_P; tb < t1; tb += CS_WAVES * CS_P) {
        float dot[CS_P][KC], hh[CS_P];
#pragma unroll
        for (int p = 0; p < CS_P; ++p) {
            hh[p] = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) dot[p][j] = 0.f;
        }
        for (int d0 = lane * 8; d0 < D; d0 += CS_TRIP) {
            float h[CS_P][8], c[8];
#pragma unroll
            for (int p = 0; p < CS_P; ++p) {
                if (tb + p < t1) {
                    ::load8(hb + (int64_t)(tb + p) * hs_t + d0, h[p]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) h[p][e] = 0.f;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) hh[p] = fmaf(h[p][e], h[p][e], hh[p]);
            }
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                if (j < nk) {
                    ::load8(cl + j * D + d0, c);
#pragma unroll
                    for (int p = 0; p < CS_P; ++p)
#pragma unroll
                        for (int e = 0; e < 8; ++e) dot[p][j] = fmaf(h[p][e], c[e], dot[p][j]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < CS_P; ++p) {
            const float hn = sqrtf(wave_sum(hh[p]));
            float mine = 0.f;
#pragma unroll
            for (int j = 0; j < KC; ++j) {
                const float d = wave_sum(dot[p][j]);
                mine = lane == j ? d : mine;
            }
            if (tb + p < t1 && lane < nk) {
                const uint32_t key = key_of<32>(mine / (hn * cn));
                best = key > best ? key : best;
            }
        }
    }
    if (lane < CS_MAX_K) wbest[wave][lane] = best;
    __syncthreads();
    if (tid < nk) {
        uint32_t m = wbest[0][tid];
#pragma unroll
        for (int w = 1; w < CS_WAVES; ++w) m = wbest[w][tid] > m ? wbest[w][tid] : m;
        part[(size_t)bs * k + j0 + tid] = m;
    }
}

// blockIdx.x = b; one wavefront, lane j = candidate j
__global__ __launch_bounds__(64) void contrastive_select_merge_kernel(const uint32_t* __restrict__ part, const float* __restrict__ probs, int32_t* __restrict__ winner,
                                                                      float* __restrict__ scores, float* __restrict__ max_sim, int splits, int k, float alpha) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    u64 c = 0;
    if (lane < k) {
        uint32_t key = 0;
        for (int s = 0; s < splits; ++s) {
            const uint32_t e = part[((size_t)b * splits + s) * k + lane];
            key = e > key ? e : key;
        }
        const float ms = (key == 0xFFFFFFFFu || key == 0) ? NAN : value_of<32>(key);
        const float score = fmaf(-alpha, ms, (1.f - alpha) * probs[b * k + lane]);
        max_sim[b * k + lane] = ms;
        scores[b * k + lane] = score;
        c = pack_top(key_of<32>(score), lane);
    }
    c = wave_max_u64(c);
    if (lane == 0) {
        const int w = (int)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFu));
        winner[b] = w >= 0 && w < k ? w : 0;
    }
}

template <class F> int by_candidates(int kc, F&& f) {
    if (kc <= 2) return f(IntC<2>{});
    if (kc <= 4) return f(IntC<4>{});
    if (kc <= 5) return f(IntC<5>{});
    if (kc <= 8) return f(IntC<8>{});
    return f(IntC<16>{});
}

template <class T, int KC> bool cs_allow_lds() {
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&contrastive_sim_kernel<T, KC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)CS_LDS_MAX) == hipSuccess;
    return ok;
}

// ------------------------------------------------------------------ commit ------------------------------------------------------------------
// item = group * bpg + block of 256 columns.  A group's columns: ccols 16-byte columns of the cache position (plane-major), then hcols of the
// hidden state, then one for the token.
template <class I>
__global__ __launch_bounds__(CS_THREADS) void contrastive_commit_kernel(unsigned char* cache, int64_t planes, int64_t Sc, int64_t row_bytes, int64_t pos,
                                                                        I* prompt, int64_t ld_prompt, int64_t index, unsigned char* hist,
                                                                        int64_t hist_b_bytes, int64_t hist_off_bytes, const unsigned char* __restrict__ cand,
                                                                        int64_t cand_row_bytes, const int32_t* __restrict__ winner, int64_t groups, int k,
                                                                        int64_t ccols, int64_t hcols, int64_t bpg) {
    const int64_t rcols = row_bytes / 16;
    for (int64_t item = blockIdx.x; item < groups * bpg; item += gridDim.x) {
        const int64_t g = item / bpg;
        int64_t col = (item % bpg) * CS_THREADS + threadIdx.x;
        const int w = winner[g];
        if (w < 0 || w >= k) continue;
        if (col < ccols) {
            const int64_t plane = col / rcols, off = (col % rcols) * 16;
            unsigned char* base = cache + ((g * k * planes + plane) * Sc + pos) * row_bytes + off;
            const int64_t cand_bytes = planes * Sc * row_bytes;
            const cs_u32x4 v = *reinterpret_cast<const cs_u32x4*>(base + (int64_t)w * cand_bytes);
            for (int j = 0; j < k; ++j)
                if (j != w) *reinterpret_cast<cs_u32x4*>(base + (int64_t)j * cand_bytes) = v;
            continue;
        }
        col -= ccols;
        if (col < hcols) {
            *reinterpret_cast<cs_u32x4*>(hist + g * hist_b_bytes + hist_off_bytes + col * 16) =
                *reinterpret_cast<const cs_u32x4*>(cand + (g * k + w) * cand_row_bytes + col * 16);
            continue;
        }
        col -= hcols;
        if (col == 0 && prompt) {
            I* base = prompt + g * k * ld_prompt + index;
            const I v = base[(int64_t)w * ld_prompt];
            for (int j = 0; j < k; ++j)
                if (j != w) base[(int64_t)j * ld_prompt] = v;
        }
    }
}

}  // namespace

extern "C" int iseg_contrastive_candidates_supported(int64_t V, int k, int dtype) {
    return (iseg_beam_select_supported(V, k, dtype) && k <= V) ? 1 : 0;
}

extern "C" int iseg_contrastive_candidates_splits(int64_t rows, int64_t V) { return iseg_beam_select_splits(rows, V); }

extern "C" size_t iseg_contrastive_candidates_scratch_bytes(int64_t rows, int64_t V, int k, int splits) {
    if (rows < 1 || !iseg_contrastive_candidates_supported(V, k, ISEG_F32)) return 0;
    return (size_t)rows * bs_resolve(rows, V, splits) * (1 + k) * sizeof(u64);
}

extern "C" int iseg_contrastive_candidates(const void* logits, int64_t ld, const int32_t* row_map, int group, float* probs, int32_t* tokens, void* ws,
                                           size_t ws_bytes, int64_t rows, int64_t V, int k, float temperature, int splits, int dtype, hipStream_t stream) {
    const char* who = "iseg_contrastive_candidates";
    ISEG_REQUIRE(logits && probs && tokens && rows > 0, "%s: bad arguments", who);
    if (!iseg_contrastive_candidates_supported(V, k, dtype)) {
        iseg_set_error("%s: needs bf16 or fp32 logits, 1 <= V <= 2^20 and 1 <= k <= min(16, V) (got V %lld, k %d, dtype %d)", who, (long long)V, k, dtype);
        return ISEG_ERR_UNSUPPORTED;
    }
    ISEG_REQUIRE(!row_map || group >= 1, "%s: a row map needs group >= 1 logits rows per output row, got %d", who, group);
    ISEG_REQUIRE(temperature > 0.f && temperature <= FLT_MAX && 1.4426950408889634f / temperature <= FLT_MAX,
                 "%s: needs a positive finite temperature (with a finite 1 / temperature), got %g", who, (double)temperature);
    ISEG_REQUIRE(ld >= V, "%s: the row pitch %lld does not cover %lld columns", who, (long long)ld, (long long)V);
    const int nsplit = bs_resolve(rows, V, splits), tiles = bs_tiles(V);
    ISEG_REQUIRE(rows * nsplit <= INT_MAX && rows * (row_map ? group : 1) <= INT_MAX, "%s: too many work items", who);
    ISEG_NEED_WORKSPACE(who, ws, ws_bytes, iseg_contrastive_candidates_scratch_bytes(rows, V, k, nsplit));
    ISEG_REQUIRE((uintptr_t)ws % 8 == 0, "%s: the scratch buffer must be 8-byte aligned", who);
    const int vec = (uintptr_t)logits % 16 == 0 && (ld * (int64_t)dtype_size(dtype)) % 16 == 0;
    const double cexp = 1.4426950408889634 / (double)temperature;
    u64* part = (u64*)ws;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((beam_select_partial_kernel<E>), dim3((unsigned)(rows * nsplit)), dim3(BS_P1_THREADS), 0, stream, (const E*)logits, ld, part,
                           1 + k, (int)V, nsplit, tiles, k, cexp, vec, row_map, group);
        hipLaunchKernelGGL((contrastive_candidates_merge_kernel<E>), dim3((unsigned)rows), dim3(64), 0, stream, probs, tokens, (const u64*)part, 1 + k,
                           nsplit, k, cexp);
        return iseg_check_launch(who);
    });
}

extern "C" int iseg_contrastive_select_supported(int64_t D, int k, int dtype) {
    return ((dtype == ISEG_BF16 || dtype == ISEG_F32) && D >= 8 && D % 8 == 0 && D <= CS_DMAX && k >= 1 && k <= CS_MAX_K) ? 1 : 0;
}

extern "C" int iseg_contrastive_select_splits(int64_t groups, int64_t index, int64_t D, int k, int dtype) {
    if (groups < 1 || index < 1 || !iseg_contrastive_select_supported(D, k, dtype)) return 0;
    return cs_splits(groups, index, cs_plan(D, k, dtype).ncg);
}

extern "C" size_t iseg_contrastive_select_scratch_bytes(int64_t groups, int64_t index, int64_t D, int k, int splits, int dtype) {
    if (groups < 1 || index < 1 || !iseg_contrastive_select_supported(D, k, dtype)) return 0;
    return (size_t)groups * cs_resolve(groups, index, cs_plan(D, k, dtype).ncg, splits) * k * sizeof(uint32_t);
}

extern "C" int iseg_contrastive_select(const void* hist, int64_t hs_b, int64_t hs_t, int64_t S, int64_t index, const void* cand, int64_t ldc,
                                       const float* probs, int32_t* winner, float* scores, float* max_sim, void* ws, size_t ws_bytes, int64_t groups,
                                       int64_t D, int k, float alpha, int splits, int dtype, hipStream_t stream) {
    const char* who = "iseg_contrastive_select";
    ISEG_REQUIRE(hist && cand && probs && winner && scores && max_sim && groups > 0, "%s: bad arguments", who);
    if (!iseg_contrastive_select_supported(D, k, dtype)) {
        iseg_set_error("%s: needs bf16 or fp32 hidden states, D a multiple of 8 in 8 .. 16384 and 1 <= k <= 16 (got D %lld, k %d, dtype %d)", who,
                       (long long)D, k, dtype);
        return ISEG_ERR_UNSUPPORTED;
    }
    ISEG_REQUIRE(index >= 1 && index <= S && S <= INT_MAX, "%s: 1 <= index <= S filled positions, got %lld of %lld", who, (long long)index, (long long)S);
    ISEG_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: 0 <= alpha <= 1, got %g", who, (double)alpha);
    ISEG_REQUIRE(hs_t >= D && hs_t % 8 == 0 && ldc >= D && ldc % 8 == 0 && (groups == 1 || hs_b >= S * hs_t) && hs_b % 8 == 0 &&
                     (uintptr_t)hist % 16 == 0 && (uintptr_t)cand % 16 == 0,
                 "%s: 16-byte aligned bases, row pitches >= D that are multiples of 8 elements, and batch rows that do not overlap", who);
    const CsPlan plan = cs_plan(D, k, dtype);
    const int nsplit = cs_resolve(groups, index, plan.ncg, splits);
    ISEG_REQUIRE(groups * nsplit * plan.ncg <= INT_MAX, "%s: too many work items", who);
    ISEG_NEED_WORKSPACE(who, ws, ws_bytes, iseg_contrastive_select_scratch_bytes(groups, index, D, k, nsplit, dtype));
    ISEG_REQUIRE((uintptr_t)ws % 4 == 0, "%s: the scratch buffer must be 4-byte aligned", who);
    uint32_t* part = (uint32_t*)ws;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        return by_candidates(plan.kc, [&](auto c) {
            constexpr int KC = decltype(c)::value;
            if (plan.lds > 48 * 1024 && !cs_allow_lds<E, KC>()) {
                iseg_set_error("%s: %zu bytes of LDS refused", who, plan.lds);
                return (int)ISEG_ERR_ARG;
            }
            hipLaunchKernelGGL((contrastive_sim_kernel<E, KC>), dim3((unsigned)(groups * nsplit * plan.ncg)), dim3(CS_THREADS), plan.lds, stream,
                               (const E*)hist, hs_b, hs_t, (const E*)cand, ldc, part, (int)index, (int)D, k, plan.kc, plan.ncg, nsplit);
            hipLaunchKernelGGL(contrastive_select_merge_kernel, dim3((unsigned)groups), dim3(64), 0, stream, (const uint32_t*)part, probs, winner, scores,
                               max_sim, nsplit, k, alpha);
            return iseg_check_launch(who);
        });
    });
}

extern "C" int iseg_contrastive_commit(void* cache, int64_t planes, int64_t Sc, int64_t row_bytes, int64_t pos, void* prompt, int64_t S, int64_t ld_prompt,
                                       int64_t index, int ids_dtype, void* hist, int64_t hs_b, int64_t hs_t, int64_t Sh, const void* cand, int64_t ldc,
                                       int64_t D, int dtype, const int32_t* winner, int64_t groups, int k, hipStream_t stream) {
    const char* who = "iseg_contrastive_commit";
    ISEG_REQUIRE(winner && groups > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(k >= 1 && k <= CS_MAX_K, "%s: 1 <= k <= 16, got %d", who, k);
    ISEG_REQUIRE(groups * k <= INT_MAX, "%s: too many rows", who);
    int64_t ccols = 0, hcols = 0;
    if (cache) {
        ISEG_REQUIRE(planes > 0 && row_bytes > 0 && row_bytes % 16 == 0 && (uintptr_t)cache % 16 == 0,
                     "%s: the cache is 16-byte aligned with rows of a multiple of 16 bytes on planes >= 1 planes (got %lld bytes, %lld planes)", who,
                     (long long)row_bytes, (long long)planes);
        ISEG_REQUIRE(pos >= 0 && pos < Sc, "%s: position %lld does not lie inside a cache of %lld", who, (long long)pos, (long long)Sc);
        ccols = planes * (row_bytes / 16);
    }
    if (prompt) {
        ISEG_REQUIRE(S > 0 && ld_prompt >= S, "%s: the prompt's row pitch is >= S", who);
        ISEG_REQUIRE(index >= 0 && index < S, "%s: position %lld does not lie inside a prompt of %lld", who, (long long)index, (long long)S);
        ISEG_REQUIRE(ids_dtype == ISEG_IDS_I32 || ids_dtype == ISEG_IDS_I64, "%s: ids_dtype %d", who, ids_dtype);
    }
    const int64_t es = (int64_t)dtype_size(dtype);
    if (hist) {
        ISEG_REQUIRE(dtype == ISEG_BF16 || dtype == ISEG_F32, "%s: dtype %d", who, dtype);
        ISEG_REQUIRE(cand && D >= 1 && (D * es) % 16 == 0 && (hs_t * es) % 16 == 0 && (hs_b * es) % 16 == 0 && (ldc * es) % 16 == 0 && hs_t >= D &&
                         ldc >= D && (groups == 1 || hs_b >= Sh * hs_t) && (uintptr_t)hist % 16 == 0 && (uintptr_t)cand % 16 == 0,
                     "%s: the hidden states are 16-byte aligned rows of a multiple of 16 bytes, pitches >= D", who);
        ISEG_REQUIRE(index >= 0 && index < Sh, "%s: position %lld does not lie inside a history of %lld", who, (long long)index, (long long)Sh);
        hcols = D * es / 16;
    }
    const int64_t bpg = ceil_div64(ccols + hcols + 1, CS_THREADS);
    const dim3 grid(grid_cap(groups * bpg, 1, CS_GRID_CAP));
    if (ids_dtype == ISEG_IDS_I64 && prompt)
        hipLaunchKernelGGL((contrastive_commit_kernel<int64_t>), grid, dim3(CS_THREADS), 0, stream, (unsigned char*)cache, planes, Sc, row_bytes, pos,
                           (int64_t*)prompt, ld_prompt, index, (unsigned char*)hist, hs_b * es, index * hs_t * es, (const unsigned char*)cand, ldc * es, winner,
                           groups, k, ccols, hcols, bpg);
    else
        hipLaunchKernelGGL((contrastive_commit_kernel<int32_t>), grid, dim3(CS_THREADS), 0, stream, (unsigned char*)cache, planes, Sc, row_bytes, pos,
                           (int32_t*)prompt, ld_prompt, index, (unsigned char*)hist, hs_b * es, index * hs_t * es, (const unsigned char*)cand, ldc * es, winner,
                           groups, k, ccols, hcols, bpg);
    return iseg_check_launch(who);
}
