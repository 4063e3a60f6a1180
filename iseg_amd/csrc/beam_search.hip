// One step of keras_nlp.samplers.BeamSampler for GemmaCausalLM.generate (compile(sampler=BeamSampler(num_beams=2)) in the class docstring of
// nlp/gemma/gemma_causal.py): the selection of the nb best of a group's nb * V candidates (iseg_beam_select) and gather_beams on the cache and
// the prompt, in place (iseg_beam_reorder).  Row g * nb + j is beam j of batch row g; include/iseg_hip.h has the full statement.
//
// Select.  Within one row the score (x - max) / T - log sum exp + log_probs[j] is a monotone function of x, so a row's candidates are its nb
// first entries in the order of order_keys.h (stored value descending, then index ascending), and the logits are read once:
//   pass 1  (topk_chunks.h, shared with contrastive.hip) one workgroup per (row, chunk of whole 2048-element tiles), four tiles in flight per trip.  Per trip: the trip's top key (wave
//           maxima through LDS); the running maximum moves to it and every thread rescales its own fp64 weight sum by exp2 in fp64 (once per
//           trip at most); the weights of the trip's 32 elements per thread, relative to the running maximum, are added in fp64; each wavefront
//           then extracts, by up to nb maxima over its lanes' packed (key, index) pairs, those of its entries that beat the workgroup's current
//           nb-th, and the first wavefront merges them with the current list.  Record: the fp64 sum, then the nb (key, index) pairs.
//   pass 2  one workgroup per group, wavefront j owns row j: the row's top key over its chunk records, the weight sum as sum_s sum_s
//           exp2((m_s - M) c) in fp64 (a lane adds its chunks in chunk order, the lanes' sums go through one butterfly), the row's nb first
//           entries by nb maxima over the records, lane r's score in fp64 rounded once.  The first wavefront then takes nb maxima over the
//           <= 256 candidates packed as (monotone key of the fp32 score, flat index).
// A weight is exp2(hi) (1 + lo ln 2) with hi + lo = (x - m) log2(e) / T formed in fp64: v_exp_f32's one ulp (2^-23 of the weight at most), the
// fma and the product (2^-24 each) are all that is lost whatever the exponent; the sum, the merge, the logarithm and the score are fp64, the
// score is rounded to fp32 once:  |error| <= 2 * 2^-23 + 2^-24 |score|.  No atomics, fixed order: a second call returns the same bits.
//
// Reorder.  The gather only moves data between the beams of one group at identical coordinates: a thread owns one 16-byte column across the
// nb beams, loads the sources of every beam whose parent is not itself, then stores.  Nothing else touches those addresses.
#include "common.h"
#include "iseg_hip.h"
#include "order_keys.h"
#include "topk_chunks.h"

#include <limits.h>
#include <math.h>
#include <utility>

namespace {

constexpr int BS_RE_THREADS = 256;
constexpr int64_t BS_RE_GRID_CAP = 16384;

typedef __attribute__((ext_vector_type(4))) unsigned int bs_u32x4;      // one 16-byte column of the cache

// blockIdx.x = group; wavefront j owns beam row j
template <class T>
__global__ __launch_bounds__(BS_P2_THREADS) void beam_select_merge_kernel(const float* __restrict__ log_probs, int32_t* __restrict__ parents,
                                                                          int32_t* __restrict__ tokens, float* __restrict__ new_log_probs,
                                                                          const u64* __restrict__ part, int pstride, int V, int splits, int nb,
                                                                          double cexp, double temperature) {
    constexpr int KB = KeyBits<T>::value;
    __shared__ u64 cand[BS_MAX_NB * BS_MAX_NB];
    const int tid = threadIdx.x, lane = tid & 63, j = tid >> 6;
    const int64_t g = blockIdx.x;
    u64 mine = 0;      // lane r < nb of wavefront j < nb: candidate r of row j as (key of the fp32 score, flat index j V + token)
    if (j < nb) {
        const u64* prow = part + (size_t)(g * nb + j) * splits * pstride;
        const uint32_t topkey = bs_row_top(prow, pstride, splits, lane);
        const float lp = log_probs[g * nb + j];
        if (!key_finite<KB>(topkey) || lp != lp) {      // the row's scores are all NaN: its first tokens
            if (lane < nb && lane < V) mine = pack_top(key_of<32>(NAN), j * V + lane);
        } else {
            const float M = value_of<KB>(topkey);
            const double lse = log(bs_row_sum<KB>(prow, pstride, splits, lane, M, cexp));
            const u64 entry = bs_row_entries(prow, pstride, splits, nb, lane);
            if (lane < nb && entry) {
                const float xv = value_of<KB>((uint32_t)(entry >> 32));
                const int idx = (int)(0xFFFFFFFFu - (uint32_t)(entry & 0xFFFFFFFFu));
                const float score = (float)((((double)xv - (double)M) / temperature - lse) + (double)lp);
                mine = pack_top(key_of<32>(score), j * V + idx);
            }
        }
    }
    if (lane < BS_MAX_NB) cand[j * BS_MAX_NB + lane] = mine;
    __syncthreads();
    if (j != 0) return;
    u64 c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = cand[lane * 4 + i];
    u64 prev = 0, out = 0;
    for (int r = 0; r < nb; ++r) {
        u64 l = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) l = (bs_open(c[i], prev, r == 0) && c[i] > l) ? c[i] : l;
        const u64 res = wave_max_u64(l);
        if (lane == r) out = res;
        prev = res;
    }
    if (lane < nb) {      // every row offers min(nb, V) candidates: there are nb at least
        const uint32_t skey = (uint32_t)(out >> 32), flat = 0xFFFFFFFFu - (uint32_t)(out & 0xFFFFFFFFu);
        int parent = (int)(flat / (uint32_t)V), token = (int)(flat % (uint32_t)V);
        if (out == 0 || parent >= nb) parent = 0, token = 0;      // not reached
        parents[g * nb + lane] = parent;
        tokens[g * nb + lane] = token;
        new_log_probs[g * nb + lane] = skey == 0xFFFFFFFFu ? NAN : value_of<32>(skey);
    }
}

// every parent of the group in [0, nb); `ident`: every beam is its own parent
__device__ __forceinline__ bool bs_parents_ok(const int32_t* __restrict__ par, int nb, bool& ident) {
    bool ok = true;
    ident = true;
    for (int j = 0; j < nb; ++j) {
        const int p = par[j];
        ok = ok && p >= 0 && p < nb;
        ident = ident && p == j;
    }
    return ok;
}

// One 16-byte column of a group: the sources of every beam whose parent is not itself, then the stores.  The beam index is a template pack, so
// the values stay in registers; the parents are read into registers before the first store.
template <int... J>
__device__ __forceinline__ void bs_gather_column(unsigned char* base, const int32_t* __restrict__ par, int nb, int64_t beam_bytes,
                                                 std::integer_sequence<int, J...>) {
    const int p[sizeof...(J)] = {(J < nb ? par[J] : J)...};
    bs_u32x4 v[sizeof...(J)];
    ((p[J] != J ? (void)(v[J] = *reinterpret_cast<const bs_u32x4*>(base + (int64_t)p[J] * beam_bytes)) : (void)0), ...);
    ((p[J] != J ? (void)(*reinterpret_cast<bs_u32x4*>(base + (int64_t)J * beam_bytes) = v[J]) : (void)0), ...);
}

// item = group * bpg + block of 256 columns; a column is 16 bytes at (plane, offset below fill) of every beam of the group
template <int NBP>
__global__ __launch_bounds__(BS_RE_THREADS) void beam_reorder_cache_kernel(unsigned char* cache, const int32_t* __restrict__ parents, int64_t groups,
                                                                           int nb, int64_t plane_bytes, int64_t beam_bytes, int64_t fill,
                                                                           int64_t ncols, int64_t bpg) {
    for (int64_t item = blockIdx.x; item < groups * bpg; item += gridDim.x) {
        const int64_t g = item / bpg, col = (item % bpg) * BS_RE_THREADS + threadIdx.x;
        const int32_t* par = parents + g * nb;
        bool ident;
        if (!bs_parents_ok(par, nb, ident) || ident || col >= ncols) continue;
        bs_gather_column(cache + g * nb * beam_bytes + (col / fill) * plane_bytes + (col % fill) * 16, par, nb, beam_bytes,
                         std::make_integer_sequence<int, NBP>{});
    }
}

// One position of a group's prompt rows: gathered by the parents; at the step's position a beam without a user token there takes its new token
template <class I, int... J>
__device__ __forceinline__ void bs_gather_position(I* base, const int32_t* __restrict__ par, int nb, int64_t ld, bool at_index,
                                                   const uint8_t* __restrict__ mask, int64_t ldm, const int32_t* __restrict__ tokens,
                                                   std::integer_sequence<int, J...>) {
    const int p[sizeof...(J)] = {(J < nb ? par[J] : 0)...};
    I v[sizeof...(J)] = {(J < nb ? base[(int64_t)p[J] * ld] : I(0))...};
    if (at_index) ((J < nb && !mask[(int64_t)J * ldm] ? (void)(v[J] = (I)tokens[J]) : (void)0), ...);
    ((J < nb ? (void)(base[(int64_t)J * ld] = v[J]) : (void)0), ...);
}

// item = group * bpg + block of 256 positions; a thread owns position s of every beam of the group
template <class I, int NBP>
__global__ __launch_bounds__(BS_RE_THREADS) void beam_reorder_prompt_kernel(I* prompt, int64_t ld, const uint8_t* __restrict__ mask, int64_t ldm,
                                                                            const int32_t* __restrict__ tokens, const int32_t* __restrict__ parents,
                                                                            int64_t groups, int nb, int64_t S, int64_t index, int64_t bpg) {
    for (int64_t item = blockIdx.x; item < groups * bpg; item += gridDim.x) {
        const int64_t g = item / bpg, s = (item % bpg) * BS_RE_THREADS + threadIdx.x;
        const int32_t* par = parents + g * nb;
        bool ident;
        if (!bs_parents_ok(par, nb, ident) || s >= S) continue;
        bs_gather_position(prompt + g * nb * ld + s, par, nb, ld, s == index, mask + g * nb * ldm + s, ldm, tokens + g * nb,
                           std::make_integer_sequence<int, NBP>{});
    }
}

// the template's beam capacity: nb rounded up to 2, 4, 8 or 16
template <class F> int by_beams(int nb, F&& f) {
    if (nb <= 2) return f(IntC<2>{});
    if (nb <= 4) return f(IntC<4>{});
    if (nb <= 8) return f(IntC<8>{});
    return f(IntC<16>{});
}

}  // namespace

extern "C" int iseg_beam_select_supported(int64_t V, int nb, int dtype) {
    return ((dtype == ISEG_BF16 || dtype == ISEG_F32) && V >= 1 && V <= BS_VMAX && nb >= 1 && nb <= BS_MAX_NB) ? 1 : 0;
}

extern "C" int iseg_beam_select_splits(int64_t rows, int64_t V) {
    if (rows < 1 || V < 1 || V > BS_VMAX) return 0;
    return bs_plan(rows, V);
}

extern "C" size_t iseg_beam_select_scratch_bytes(int64_t rows, int64_t V, int nb, int splits) {
    if (rows < 1 || !iseg_beam_select_supported(V, nb, ISEG_F32)) return 0;
    return (size_t)rows * bs_resolve(rows, V, splits) * (1 + nb) * sizeof(u64);
}

extern "C" int iseg_beam_select(const void* logits, int64_t ld, const float* log_probs, int32_t* parents, int32_t* tokens, float* new_log_probs, void* ws,
                                size_t ws_bytes, int64_t rows, int64_t V, int nb, float temperature, int splits, int dtype, hipStream_t stream) {
    const char* who = "iseg_beam_select";
    ISEG_REQUIRE(logits && log_probs && parents && tokens && new_log_probs && rows > 0, "%s: bad arguments", who);
    if (!iseg_beam_select_supported(V, nb, dtype)) {
        iseg_set_error("%s: needs bf16 or fp32 logits, 1 <= V <= 2^20 and 1 <= nb <= 16 (got V %lld, nb %d, dtype %d)", who, (long long)V, nb, dtype);
        return ISEG_ERR_UNSUPPORTED;
    }
    ISEG_REQUIRE(rows % nb == 0, "%s: %lld rows are no whole number of groups of %d beams", who, (long long)rows, nb);
    ISEG_REQUIRE(temperature > 0.f && temperature <= FLT_MAX && 1.4426950408889634f / temperature <= FLT_MAX,
                 "%s: needs a positive finite temperature (with a finite 1 / temperature), got %g", who, (double)temperature);
    ISEG_REQUIRE(ld >= V, "%s: the row pitch %lld does not cover %lld columns", who, (long long)ld, (long long)V);
    const int nsplit = bs_resolve(rows, V, splits), tiles = bs_tiles(V);
    ISEG_REQUIRE(rows * nsplit <= INT_MAX, "%s: too many work items", who);
    ISEG_NEED_WORKSPACE(who, ws, ws_bytes, iseg_beam_select_scratch_bytes(rows, V, nb, nsplit));
    ISEG_REQUIRE((uintptr_t)ws % 8 == 0, "%s: the scratch buffer must be 8-byte aligned", who);
    const int vec = (uintptr_t)logits % 16 == 0 && (ld * (int64_t)dtype_size(dtype)) % 16 == 0;
    const double cexp = 1.4426950408889634 / (double)temperature;
    u64* part = (u64*)ws;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((beam_select_partial_kernel<E>), dim3((unsigned)(rows * nsplit)), dim3(BS_P1_THREADS), 0, stream, (const E*)logits, ld, part,
                           1 + nb, (int)V, nsplit, tiles, nb, cexp, vec, (const int32_t*)nullptr, 1);
        hipLaunchKernelGGL((beam_select_merge_kernel<E>), dim3((unsigned)(rows / nb)), dim3(BS_P2_THREADS), 0, stream, log_probs, parents, tokens,
                           new_log_probs, (const u64*)part, 1 + nb, (int)V, nsplit, nb, cexp, (double)temperature);
        return iseg_check_launch(who);
    });
}

extern "C" int iseg_beam_reorder(void* cache, int64_t planes, int64_t Sc, int64_t row_bytes, int64_t len, void* prompt, int64_t S, int64_t ld_prompt,
                                 const uint8_t* mask, int64_t ld_mask, const int32_t* tokens, int64_t index, int ids_dtype, const int32_t* parents,
                                 int64_t groups, int nb, hipStream_t stream) {
    const char* who = "iseg_beam_reorder";
    ISEG_REQUIRE(parents && groups > 0, "%s: bad arguments", who);
    ISEG_REQUIRE(nb >= 1 && nb <= BS_MAX_NB, "%s: 1 <= nb <= 16, got %d", who, nb);
    ISEG_REQUIRE(groups * nb <= INT_MAX, "%s: too many rows", who);
    if (cache) {
        ISEG_REQUIRE(planes > 0 && row_bytes > 0 && row_bytes % 16 == 0 && (uintptr_t)cache % 16 == 0,
                     "%s: the cache is 16-byte aligned with rows of a multiple of 16 bytes on planes >= 1 planes (got %lld bytes, %lld planes)", who,
                     (long long)row_bytes, (long long)planes);
        ISEG_REQUIRE(Sc > 0 && len >= 0 && len <= Sc, "%s: %lld filled positions do not lie inside a cache of %lld", who, (long long)len, (long long)Sc);
    }
    if (prompt) {
        ISEG_REQUIRE(S > 0 && mask && tokens && ld_prompt >= S && ld_mask >= S, "%s: the prompt needs its mask and tokens, and row pitches >= S", who);
        ISEG_REQUIRE(index >= 0 && index < S, "%s: position %lld does not lie inside a prompt of %lld", who, (long long)index, (long long)S);
        ISEG_REQUIRE(ids_dtype == ISEG_IDS_I32 || ids_dtype == ISEG_IDS_I64, "%s: ids_dtype %d", who, ids_dtype);
    }
    return by_beams(nb, [&](auto c) {
        constexpr int NBP = decltype(c)::value;
        if (cache && len > 0) {
            const int64_t fill = len * (row_bytes / 16), ncols = planes * fill, bpg = ceil_div64(ncols, BS_RE_THREADS);
            hipLaunchKernelGGL((beam_reorder_cache_kernel<NBP>), dim3(grid_cap(groups * bpg, 1, BS_RE_GRID_CAP)), dim3(BS_RE_THREADS), 0, stream,
                               (unsigned char*)cache, parents, groups, nb, Sc * row_bytes, planes * Sc * row_bytes, fill, ncols, bpg);
        }
        if (prompt) {
            const int64_t bpg = ceil_div64(S, BS_RE_THREADS);
            const dim3 grid(grid_cap(groups * bpg, 1, BS_RE_GRID_CAP));
            if (ids_dtype == ISEG_IDS_I32)
                hipLaunchKernelGGL((beam_reorder_prompt_kernel<int32_t, NBP>), grid, dim3(BS_RE_THREADS), 0, stream, (int32_t*)prompt, ld_prompt, mask,
                                   ld_mask, tokens, parents, groups, nb, S, index, bpg);
            else
                hipLaunchKernelGGL((beam_reorder_prompt_kernel<int64_t, NBP>), grid, dim3(BS_RE_THREADS), 0, stream, (int64_t*)prompt, ld_prompt, mask,
                                   ld_mask, tokens, parents, groups, nb, S, index, bpg);
        }
        return iseg_check_launch(who);
    });
}
