// The commit of one decoding step (sample_loop of iseg_amd/nlp/samplers.py, keras_nlp Sampler.__call__): what the host loop does between the
// sampler's choice and the next forward pass, on state that lives in device memory, so that a whole step is one replayed graph.
//
//   state   prompt [B, S] ids, mask [B, S] bytes (non-zero = user token), pos_d: the index of the previous token (generate_step's
//           cache_update_index), cur_ids [B]: the token the next step embeds, done [B] bytes, tokens [B]: the sampler's choice.
//   launch  p = *pos_d.  If p + 1 lies outside [0, S), or end_token_id >= 0 and every done[b] is set, NOTHING is written (the freeze: replays
//           past the end of the generation are harmless).  Otherwise, per row b:
//               t = mask[b, p + 1] ? prompt[b, p + 1] : tokens[b];  prompt[b, p + 1] = t;  cur_ids[b] = t;
//               done[b] |= (t == end_token_id && !mask[b, p + 1]);
//           and then *pos_d = p + 1.
// One workgroup loops over the rows (any B); every thread reads p before the first barrier, the all-done flag is reduced through LDS, and
// one thread writes *pos_d after the last barrier.  Plain loads and vector stores, no atomics.
#include "common.h"
#include "iseg_hip.h"

#include <limits.h>

namespace {

constexpr int DC_THREADS = 256;

template <class I, class K>
__global__ __launch_bounds__(DC_THREADS) void decode_commit_kernel(I* __restrict__ prompt, int64_t ldp, const uint8_t* __restrict__ mask, int64_t ldm,
                                                                   int32_t* __restrict__ pos_d, I* __restrict__ cur_ids, uint8_t* __restrict__ done,
                                                                   const K* __restrict__ tokens, int64_t batch, int S, int64_t end_token_id) {
    __shared__ int all_done;
    const int p = *pos_d;
    if (threadIdx.x == 0) all_done = 1;
    __syncthreads();      // every thread holds p; the flag is initialised
    const bool live = p >= -1 && p < S - 1;
    if (live && end_token_id >= 0) {
        bool mine = true;
        for (int64_t b = threadIdx.x; b < batch; b += DC_THREADS) mine = mine && done[b] != 0;
        if (!mine) all_done = 0;      // every writer stores the same value
    }
    __syncthreads();
    if (!live || (end_token_id >= 0 && all_done)) return;      // the same decision in every thread
    const int64_t col = (int64_t)p + 1;
    for (int64_t b = threadIdx.x; b < batch; b += DC_THREADS) {
        const bool user = mask[b * ldm + col] != 0;
        const I t = user ? prompt[b * ldp + col] : (I)tokens[b];
        prompt[b * ldp + col] = t;
        cur_ids[b] = t;
        if (!user && end_token_id >= 0 && (int64_t)t == end_token_id) done[b] = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) *pos_d = p + 1;
}

template <class I>
int launch_ids(void* prompt, int64_t ldp, const uint8_t* mask, int64_t ldm, int32_t* pos_d, void* cur_ids, uint8_t* done, const void* tokens,
               int64_t batch, int S, int64_t end_token_id, int tokens_dtype, hipStream_t stream) {
    if (tokens_dtype == ISEG_IDS_I64)
        hipLaunchKernelGGL((decode_commit_kernel<I, int64_t>), dim3(1), dim3(DC_THREADS), 0, stream, (I*)prompt, ldp, mask, ldm, pos_d, (I*)cur_ids, done,
                           (const int64_t*)tokens, batch, S, end_token_id);
    else
        hipLaunchKernelGGL((decode_commit_kernel<I, int32_t>), dim3(1), dim3(DC_THREADS), 0, stream, (I*)prompt, ldp, mask, ldm, pos_d, (I*)cur_ids, done,
                           (const int32_t*)tokens, batch, S, end_token_id);
    return iseg_check_launch("iseg_decode_commit");
}

}  // namespace

extern "C" int iseg_decode_commit(void* prompt, int64_t ld_prompt, const uint8_t* mask, int64_t ld_mask, int32_t* pos_d, void* cur_ids, uint8_t* done,
                                  const void* tokens, int64_t batch, int S, int64_t end_token_id, int ids_dtype, int tokens_dtype,
                                  hipStream_t stream) {
    const char* who = "iseg_decode_commit";
    ISEG_REQUIRE(prompt && mask && pos_d && cur_ids && done && tokens && batch > 0 && S > 0 && S < INT_MAX, "%s: bad arguments", who);
    ISEG_REQUIRE(ld_prompt >= S && ld_mask >= S, "%s: row pitches must cover their rows", who);
    ISEG_REQUIRE((ids_dtype == ISEG_IDS_I32 || ids_dtype == ISEG_IDS_I64) && (tokens_dtype == ISEG_IDS_I32 || tokens_dtype == ISEG_IDS_I64),
                 "%s: ids and tokens are int32 (ISEG_IDS_I32) or int64 (ISEG_IDS_I64), got codes %d and %d", who, ids_dtype, tokens_dtype);
    const uintptr_t ids_align = ids_dtype == ISEG_IDS_I64 ? 8 : 4, tok_align = tokens_dtype == ISEG_IDS_I64 ? 8 : 4;
    ISEG_REQUIRE(((uintptr_t)prompt | (uintptr_t)cur_ids) % ids_align == 0 && (uintptr_t)tokens % tok_align == 0 && (uintptr_t)pos_d % 4 == 0,
                 "%s: operands must be aligned to their element size", who);
    if (ids_dtype == ISEG_IDS_I64)
        return launch_ids<int64_t>(prompt, ld_prompt, mask, ld_mask, pos_d, cur_ids, done, tokens, batch, S, end_token_id, tokens_dtype, stream);
    return launch_ids<int32_t>(prompt, ld_prompt, mask, ld_mask, pos_d, cur_ids, done, tokens, batch, S, end_token_id, tokens_dtype, stream);
}
