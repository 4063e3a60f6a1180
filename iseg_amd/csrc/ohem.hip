// Online hard example mining for the ignore-label cross-entropy (losses/ohem.py:11-39 ohem_selector of the reference, restated literally).
//
//   thresh given:  prob_p = max_c softmax(z_p)_c * onehot_pc  (the labelled class's probability, 0 on a zero row);  nnz = #{prob != 0};
//                  k = min(min_kept * batch, nnz - 1);  min_threshold = sort(prob, DESCENDING)[k]  (0 when nnz == 0);
//                  threshold = max(min_threshold, thresh);  out_p = prob_p < threshold ? loss_p : 0
//   thresh None:   threshold = sort(loss, DESCENDING)[min_kept * batch];  out_p = loss_p > threshold ? loss_p : 0
// The threshold only enters comparisons, so d(out)/d(logits) is the loss's own gradient on kept pixels and 0 elsewhere: `keep` is the
// grad_px of iseg_softmax_ce_ignore.
//
// The reference sorts all N*H*W values.  Here the k-th largest value comes from a most-significant-digit radix select: four 8-bit passes over
// the order-preserving unsigned image of the float bits (sign bit flipped for non-negatives, every bit for negatives).  A pass bins the values
// that still match the digits chosen so far -- one LDS histogram per workgroup, flushed with one integer atomic per non-empty bin -- and a
// one-workgroup launch then walks the 256 counts from the top, picks the digit that holds the wanted rank and carries the rest of the rank on.
// The rank lives on the device (it depends on nnz).  Every dependency between workgroups is a launch boundary; integer atomics only; the masked
// sum is reduced in two stages in a fixed order.  No host read, no copy, no allocation: the call captures into a graph and is bit-reproducible.
#include "common.h"
#include "ce_rows.h"
#include "iseg_hip.h"

namespace {

// int32 state block: four histograms of 256 bins, then the counters
constexpr int ST_NNZ = 1024, ST_RANK = 1025, ST_PREFIX = 1026;
static_assert(ST_PREFIX < ISEG_OHEM_STATE_INTS, "state block too small");
constexpr int MAX_BLOCKS = ISEG_OHEM_PARTIAL_FLOATS;      // grid cap of the streaming passes = length of the partial-sum block
constexpr int PER_BLOCK = 1024;                           // values per workgroup before the grid-stride loop takes a second trip

__device__ __forceinline__ unsigned ordered_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void ohem_label_prob_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int64_t P,
                                                              int C, int ignore, float* __restrict__ prob, int pix) {
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [pix][C]
    const int64_t ntiles = (P + pix - 1) / pix;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        __syncthreads();      // previous tile fully consumed
        const int64_t p0 = tl * pix;
        const int npx = (int)((P - p0 < pix) ? (P - p0) : pix);
        stage_rows(tile, logits + p0 * C, p0 * C, (int64_t)npx * C);
        __syncthreads();
        if ((int)threadIdx.x < npx) {
            const float* z = tile + threadIdx.x * C;
            int y = labels[p0 + threadIdx.x];
            const bool in_range = label_class(y, ignore, C);
            float mx = z[0];
            for (int c = 1; c < C; ++c)
                if (z[c] > mx) mx = z[c];
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += __expf(z[c] - mx);      // the sum softmax_ce_kernel takes, in its order
            prob[p0 + threadIdx.x] = in_range ? __expf(z[y] - mx) / se : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void ohem_zero_kernel(int32_t* __restrict__ state) {
    for (int i = threadIdx.x; i < ISEG_OHEM_STATE_INTS; i += 256) state[i] = 0;
}

// pass 0..3: bins digit `pass` (most significant first) of the values whose higher digits equal the prefix picked so far; pass 0 also counts
// the non-zero values.  Scalar loads: the pass is bound by the LDS atomics (probabilities crowd into a few exponents), not by its 4 P bytes.
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ values, int64_t P, int pass, int32_t* __restrict__ state) {
    __shared__ unsigned hist[256];
    __shared__ unsigned nonzero;
    hist[threadIdx.x] = 0u;
    if (threadIdx.x == 0) nonzero = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned high = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
    const unsigned prefix = pass ? (unsigned)state[ST_PREFIX] : 0u;
    unsigned nz = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const float v = values[i];
        const unsigned key = ordered_key(v);
        if ((key & high) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        nz += v != 0.f;
    }
    if (pass == 0 && nz) atomicAdd(&nonzero, nz);
    __syncthreads();
    unsigned* global_hist = reinterpret_cast<unsigned*>(state) + pass * 256;
    if (hist[threadIdx.x]) atomicAdd(&global_hist[threadIdx.x], hist[threadIdx.x]);      // integer counts: order-independent, exact
    if (pass == 0 && threadIdx.x == 0 && nonzero) atomicAdd(reinterpret_cast<unsigned*>(state) + ST_NNZ, nonzero);
}

// one workgroup: the digit d of this pass with  #{bins above d} <= rank < #{bins d and above}  (descending order), the rank inside bin d.
// Pass 0 sets the rank (prob mode: min(min_kept_total, nnz - 1)); pass 3 ends with the whole key and writes threshold_out / nnz_out.
__global__ __launch_bounds__(256) void ohem_pick_kernel(int pass, int prob_mode, int64_t min_kept_total, float thresh, int32_t* __restrict__ state,
                                                        float* __restrict__ threshold_out, int32_t* __restrict__ nnz_out) {
    __shared__ unsigned s[256];
    const int t = threadIdx.x;
    const unsigned count = (unsigned)state[pass * 256 + t];
    const int nnz = state[ST_NNZ];
    const bool empty = prob_mode && nnz == 0;      // no labelled pixel at all: min_threshold = 0 (the walk below still runs, on rank 0)
    unsigned rank;
    if (pass > 0) rank = (unsigned)state[ST_RANK];
    else if (!prob_mode) rank = (unsigned)min_kept_total;
    else rank = empty ? 0u : (unsigned)(min_kept_total < (int64_t)nnz - 1 ? min_kept_total : (int64_t)nnz - 1);
    const unsigned prefix = pass ? (unsigned)state[ST_PREFIX] : 0u;
    s[t] = count;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {      // s[t] = count[t] + count[t + 1] + ... + count[255]
        const unsigned v = t + o < 256 ? s[t + o] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const unsigned above = s[t] - count;
    if (above <= rank && rank < s[t]) {      // exactly one thread: the counts of a pass add up to more than its rank
        const unsigned key = prefix | ((unsigned)t << (24 - 8 * pass));
        state[ST_RANK] = (int32_t)(rank - above);
        state[ST_PREFIX] = (int32_t)key;
        if (pass == 3) {
            const float selected = empty ? 0.f : key_value(key);
            threshold_out[0] = prob_mode ? fmaxf(selected, thresh) : selected;
            nnz_out[0] = nnz;
        }
    }
}

// keep_p = values_p < threshold (prob mode) or values_p > threshold (loss mode), strict; loss_out_p = keep_p ? loss_p : 0; the workgroup's
// sum of loss_out in a fixed order (thread: its grid-stride elements in order; wavefront: xor butterfly; workgroup: four wavefronts in order)
__global__ __launch_bounds__(256) void ohem_apply_kernel(const float* values, const float* loss, int64_t P, int prob_mode,
                                                         const float* __restrict__ threshold, float* __restrict__ keep, float* loss_out,
                                                         float* __restrict__ partials) {
    __shared__ float wsum[4];
    const float thr = threshold[0];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const float v = values[i];
        const bool k = prob_mode ? v < thr : v > thr;
        keep[i] = k ? 1.f : 0.f;
        if (loss) {
            const float l = k ? loss[i] : 0.f;
            if (loss_out) loss_out[i] = l;
            acc += l;
        }
    }
    if (partials) {
        const float w = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
        __syncthreads();
        if (threadIdx.x == 0) partials[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

__global__ __launch_bounds__(256) void ohem_sum_kernel(const float* __restrict__ partials, int n, float* __restrict__ out, float scale) {
    // single workgroup, fixed-order tree -> deterministic
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0] * scale;
}

}  // namespace

extern "C" int iseg_ohem_label_prob(const float* logits, const int32_t* labels, int64_t P, int C, int ignore_label, float* prob,
                                    hipStream_t stream) {
    ISEG_REQUIRE(logits && labels && prob, "iseg_ohem_label_prob: null logits, labels or prob");
    ISEG_REQUIRE(P >= 1 && P <= INT32_MAX, "iseg_ohem_label_prob: %lld positions (1..2^31-1)", (long long)P);
    ISEG_REQUIRE(C >= 1 && C <= 256, "iseg_ohem_label_prob: num_class %d (1..256: one 64-pixel tile of fp32 logits must fit 64 KiB of LDS)", C);
    const int pix = pixels_per_block(C);
    const unsigned grid = grid_cap(P, pix, 2048);
    hipLaunchKernelGGL(ohem_label_prob_kernel, dim3(grid), dim3(256), (size_t)pix * C * sizeof(float), stream, logits, labels, P, C, ignore_label,
                       prob, pix);
    return iseg_check_launch("iseg_ohem_label_prob");
}

extern "C" int iseg_ohem_select(const float* values, const float* loss, int64_t P, int64_t min_kept_total, float thresh, int values_are_loss,
                                float* keep, float* loss_out, float* masked_sum, float sum_scale, float* threshold_out, int32_t* nnz_out,
                                int32_t* state, float* partials, hipStream_t stream) {
    ISEG_REQUIRE(values && keep && threshold_out && nnz_out && state, "iseg_ohem_select: null values, keep, threshold_out, nnz_out or state");
    ISEG_REQUIRE(loss || (!loss_out && !masked_sum), "iseg_ohem_select: loss_out and masked_sum need loss");
    ISEG_REQUIRE(partials || !masked_sum, "iseg_ohem_select: masked_sum needs the partial-sum block");
    ISEG_REQUIRE(P >= 1 && P <= INT32_MAX, "iseg_ohem_select: %lld positions (1..2^31-1: the counters are int32)", (long long)P);
    ISEG_REQUIRE(values != keep && loss != keep && (!loss_out || loss_out != keep),
                 "iseg_ohem_select: keep is written while values and loss are read, it cannot be values, loss or loss_out");
    ISEG_REQUIRE(min_kept_total >= 0, "iseg_ohem_select: min_kept_total %lld < 0", (long long)min_kept_total);
    ISEG_REQUIRE(!values_are_loss || min_kept_total < P, "iseg_ohem_select: index %lld of %lld sorted losses", (long long)min_kept_total,
                 (long long)P);
    const int prob_mode = values_are_loss ? 0 : 1;
    const unsigned grid = grid_cap(P, PER_BLOCK, MAX_BLOCKS);
    hipLaunchKernelGGL(ohem_zero_kernel, dim3(1), dim3(256), 0, stream, state);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(ohem_hist_kernel, dim3(grid), dim3(256), 0, stream, values, P, pass, state);
        hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(256), 0, stream, pass, prob_mode, min_kept_total, thresh, state, threshold_out, nnz_out);
    }
    hipLaunchKernelGGL(ohem_apply_kernel, dim3(grid), dim3(256), 0, stream, values, loss, P, prob_mode, (const float*)threshold_out, keep, loss_out,
                       masked_sum ? partials : nullptr);
    if (masked_sum) hipLaunchKernelGGL(ohem_sum_kernel, dim3(1), dim3(256), 0, stream, (const float*)partials, (int)grid, masked_sum, sum_scale);
    return iseg_check_launch("iseg_ohem_select");
}
