// Gemma with a key/value cache (nlp/gemma/gemma_attention.py:161-179 and :116-151 under the mask of gemma_decoder_block.py:114-136 with a cache):
// the rotary embedding that writes straight into the cache, and attention of a few new tokens over the cache.
//
// Decode attention.  The new tokens sit at positions pos0 .. pos0 + Tn - 1; key s is visible to new token t iff s <= pos0 + t (call_with_cache
// passes no padding mask).  The g = nq / nkv query heads of one key/value head are stacked with the Tn tokens as g * Tn <= 16 query rows of ONE
// problem (row t * g + j, as gemma.hip): they fill the sixteen columns of one v_mfma_f32_16x16x32_bf16 tile and K / V are read once per group.
// With so few rows the only parallelism left is along the cache, so the visible keys (pos0 + Tn of them, in tiles of 64) are cut into `splits`
// chunks of whole tiles:
//   pass 1  one workgroup per (sample, kv head, chunk), one wavefront per 64-column value slab (h / 64 of them).  The wavefronts share the
//           chunk's scores S^T = K Q^T (keys on MFMA rows, query rows on columns): each computes the 16-key groups that fall to it from K
//           fragments loaded straight from global memory to registers, so K is read once per workgroup, and hands them on through LDS.  Every
//           wavefront then walks the online softmax over the tile and accumulates its 64 columns of O^T = V^T P^T (V through a wave-private
//           LDS image and ds_read_b64_tr_b16).  The next tile's K fragments and V rows are in flight while a tile is worked on.  It leaves,
//           per stacked row, an UNNORMALISED fp32 partial in the caller's workspace: the running maximum m, the sum l and the h accumulators.
//   pass 2  one workgroup per stacked row merges the partials in chunk order: out = sum_s w_s o_s / sum_s w_s l_s, w_s = exp2(c (m_s - M)),
//           M = max_s m_s, and rounds once to bf16.
// Masking is gemma.hip's: a masked score never enters the maximum and its probability is the constant 0; a row that has seen nothing in a chunk
// keeps m = -FLT_MAX and l = 0, and the merge gives such a partial the factor 0 without forming an exp2 of a difference of sentinels.  Keys
// past pos0 + Tn - 1 are never loaded (zero fragments): the cache behind the write position may hold anything.  No atomics, fixed order: a second
// call is bit-identical.
//
// The _at entry points (iseg_gemma_rope_cache_at, iseg_gemma_decode_attention_at) read the position from ONE int32 in device memory when the
// kernels run, so that a captured graph of a decoding step can be replayed at every position.  The grid and the workspace are those of the
// cache's capacity (the plan at pos0 = S - Tn); every workgroup derives the tile count and the effective chunk count of *pos_d with the
// functions the host launcher plans with (visible_tiles, resolve_splits), workgroups of pass 1 past the effective count return at once and
// pass 2 merges the effective chunks alone, in chunk order: the arithmetic is the host-position launcher's at pos0 = *pos_d, bit for bit.
// A position outside [0, S - Tn] makes every workgroup return before it reads or writes anything else.
#include "attn_tile.h"
#include "iseg_hip.h"

#include <limits.h>

namespace {

using namespace attn;

constexpr int DROWS = 16;        // stacked query rows of one problem: the columns of one MFMA tile
constexpr int DH_MAX = 256;
constexpr int DPART_HEAD = 2 * DROWS;      // floats in front of a partial's accumulators: m[16] | l[16]
constexpr int SSTRIDE = AK + 4;            // row stride (floats) of the LDS score image [query row][key]: 272-B rows

// ---- the split plan, on both sides: the host launchers size grids and workspaces with it, the _at kernels derive it from *pos_d ------------
__host__ __device__ inline int visible_tiles(int pos0, int Tn) { return (int)(((int64_t)pos0 + Tn + AK - 1) / AK); }

// chunks of the launcher's own plan: enough workgroups for two per CU of a 256-CU chip, at least two key tiles per chunk
__host__ __device__ inline int plan_splits(int64_t batch, int pos0, int Tn, int nkv) {
    const int64_t groups = batch * nkv, div = groups < 1 ? 1 : groups, want = (512 + div - 1) / div, most = visible_tiles(pos0, Tn) / 2;
    return (int)(want < most ? want : most < 1 ? 1 : most);
}

__host__ __device__ inline int resolve_splits(int64_t batch, int pos0, int Tn, int nkv, int splits) {
    if (splits <= 0) return plan_splits(batch, pos0, Tn, nkv);
    const int tiles = visible_tiles(pos0, Tn);
    return splits < tiles ? splits : tiles;
}

__device__ __forceinline__ bf16x8 qfrag(const bf16_t* __restrict__ base, int64_t off, int col) {
    if (off < 0) return zero8();
    return *reinterpret_cast<const bf16x8*>(base + off + col);
}

// blockIdx.x = ((b * nkv) + kvh) * splits + split.  A partial is DPART_HEAD + GT * H floats.  Wavefront w of the SLABS = H / 64 computes the
// scores of the 16-key groups w, w + SLABS, .. of a tile over the whole head width and leaves them in LDS; after one barrier every wavefront
// reads all 64 keys' scores back in the accumulator layout, repeats the (cheap) softmax and multiplies into ITS 64 value columns.  The score
// buffer is double: the barrier of tile k + 1 orders the reads of tile k before the writes of tile k + 2.
// AT: pos0 is *pos_d (in [0, max_pos], or every thread returns), `splits` is the grid's chunk count (the capacity's plan, also the stride of a
// group's partials) and `splits_arg` the caller's argument, from which the effective count `nsplit` of this position is resolved.
template <int SLABS, bool AT>
__global__ __launch_bounds__(64 * SLABS) void gemma_decode_partial_kernel(const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ kc,
                                                                          int64_t kbs, int64_t ldk, const bf16_t* __restrict__ vc, int64_t vbs,
                                                                          int64_t ldv, float* __restrict__ part, int Tn, int pos0, int nkv, int g,
                                                                          int splits, int tiles, float scale, const int32_t* __restrict__ pos_d,
                                                                          int max_pos, int64_t batch, int splits_arg) {
    constexpr int H = SLABS * AD;
    int nsplit = splits;
    if constexpr (AT) {
        pos0 = *pos_d;
        if (pos0 < 0 || pos0 > max_pos) return;
        tiles = visible_tiles(pos0, Tn);
        nsplit = resolve_splits(batch, pos0, Tn, nkv, splits_arg);
        if ((int)(blockIdx.x % splits) >= nsplit) return;
    }
    constexpr int TJ = (4 + SLABS - 1) / SLABS;      // 16-key groups of a tile per wavefront
    __shared__ __attribute__((aligned(16))) bf16_t Vimg[SLABS][AK * ASTRIDE];
    __shared__ __attribute__((aligned(16))) float Simg[2][DROWS * SSTRIDE];
    const int lane = threadIdx.x & 63, slab = threadIdx.x >> 6;
    bf16_t* Vl = Vimg[slab];
    int64_t item = blockIdx.x;
    const int split = (int)(item % splits);
    item /= splits;
    const int kvh = (int)(item % nkv);
    const int64_t b = item / nkv;
    const int GT = g * Tn, nvis = pos0 + Tn;
    const int jl = lane & 15, g4 = (lane >> 4) * 4, c8 = 8 * (lane >> 4);
    const float c = scale * LOG2E;
    const int vrow = lane >> 3, vcol = (lane & 7) * 8;

    const bf16_t* qb = q + b * Tn * ldq + (int64_t)kvh * g * H;
    const bf16_t* kb = kc + b * kbs + (int64_t)kvh * H;
    const bf16_t* vb = vc + b * vbs + (int64_t)kvh * H + slab * AD;

    // this lane's query column: stacked row jl = token jl / g, head jl % g of the group; past the last row it sees nothing
    const int tok = jl / g;
    const int64_t qoff = jl < GT ? (int64_t)tok * ldq + (int64_t)(jl - tok * g) * H : -1;
    const int tq = jl < GT ? pos0 + tok : -1;
    bf16x8 aq[H / 32];
#pragma unroll
    for (int ks = 0; ks < H / 32; ++ks) aq[ks] = qfrag(qb, qoff, ks * 32 + c8);

    f32x4 o[4];      // [td]: O[row jl][column slab * 64 + td * 16 + g4 + r]
#pragma unroll
    for (int td = 0; td < 4; ++td) o[td] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -FLT_MAX, l = 0.f;

    // K fragments of this wavefront's key groups and its V rows, straight to registers, one tile ahead of their use
    bf16x8 kf[TJ][H / 32], vr[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < TJ; ++i)
            if (slab + i * SLABS < 4) {
#pragma unroll
                for (int ks = 0; ks < H / 32; ++ks) kf[i][ks] = gfrag(kb, ldk, k0 + (slab + i * SLABS) * 16 + jl, nvis, ks * 32, lane);
            }
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) vr[cc] = grow8(vb, ldv, k0 + vrow + 8 * cc, nvis, vcol);
    };
    const int t0 = (int)((int64_t)split * tiles / nsplit), t1 = (int)((int64_t)(split + 1) * tiles / nsplit);
    fetch(t0 * AK);
    for (int kt = t0; kt < t1; ++kt) {
        const int k0 = kt * AK;
        float* Sl = Simg[(kt - t0) & 1];
#pragma unroll
        for (int i = 0; i < TJ; ++i)
            if (slab + i * SLABS < 4) {      // keys k0 + tj * 16 + g4 + r of group tj = slab + i * SLABS, query row jl
                f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < H / 32; ++ks) st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[i][ks], aq[ks], st, 0, 0, 0);
                *reinterpret_cast<f32x4*>(Sl + jl * SSTRIDE + (slab + i * SLABS) * 16 + g4) = st;
            }
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) *reinterpret_cast<bf16x8*>(Vl + (vrow + 8 * cc) * ASTRIDE + vcol) = vr[cc];
        if (kt + 1 < t1) fetch(k0 + AK);
        __syncthreads();
        f32x4 s[4];      // [tj]: key k0 + tj * 16 + g4 + r, query row jl
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) s[tj] = *reinterpret_cast<const f32x4*>(Sl + jl * SSTRIDE + tj * 16 + g4);

        float mx = -FLT_MAX;
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k0 + tj * 16 + g4 + r <= tq) mx = fmaxf(mx, s[tj][r]);
        mx = fmaxf(mx, xorf(mx, 16));
        mx = fmaxf(mx, xorf(mx, 32));
        const float mnew = fmaxf(m, mx);
        // nothing visible so far (sentinel): no exp2 of a sentinel difference; l and o are still zero
        const float alpha = m == -FLT_MAX ? 0.f : __builtin_amdgcn_exp2f((m - mnew) * c);
        const float mc = mnew == -FLT_MAX ? 0.f : mnew * c;
        m = mnew;
        float sum = 0.f;
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = k0 + tj * 16 + g4 + r <= tq ? recompute_p(s[tj][r], c, mc) : 0.f;
                s[tj][r] = pv;
                sum += pv;
            }
        l = l * alpha + sum;      // per-lane partial over this lane's keys; the four key groups are summed once at the end
#pragma unroll
        for (int td = 0; td < 4; ++td)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[td][r] *= alpha;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 bp = pack_b(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
            for (int td = 0; td < 4; ++td)
                o[td] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ltfrag(Vl, 32 * ks, 32 * ks + 16, td * 16, lane), bp, o[td], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    l += xorf(l, 16);
    l += xorf(l, 32);
    if (jl < GT) {
        float* p = part + (int64_t)blockIdx.x * (DPART_HEAD + GT * H);
        if (slab == 0 && g4 == 0) {
            p[jl] = m;
            p[DROWS + jl] = l;
        }
        float* acc = p + DPART_HEAD + jl * H + slab * AD + g4;
#pragma unroll
        for (int td = 0; td < 4; ++td) *reinterpret_cast<float4*>(acc + td * 16) = float4{o[td][0], o[td][1], o[td][2], o[td][3]};
    }
}

// blockIdx.x = ((b * nkv) + kvh) * GT + R: one stacked row, a thread per column; the partials are merged in chunk order.
// AT: `splits` is the stride of a group's partials (the capacity's plan); the chunks merged are the `nsplit` of the position *pos_d
template <bool AT>
__global__ __launch_bounds__(256) void gemma_decode_merge_kernel(const float* __restrict__ part, bf16_t* __restrict__ out, int64_t ldo, int Tn, int nkv,
                                                                 int g, int h, int splits, float scale, const int32_t* __restrict__ pos_d,
                                                                 int max_pos, int64_t batch, int splits_arg) {
    int nsplit = splits;
    if constexpr (AT) {
        const int pos0 = *pos_d;
        if (pos0 < 0 || pos0 > max_pos) return;
        nsplit = resolve_splits(batch, pos0, Tn, nkv, splits_arg);
    }
    const int GT = g * Tn;
    const int R = (int)(blockIdx.x % GT);
    const int64_t grp = blockIdx.x / GT;
    const int kvh = (int)(grp % nkv);
    const int64_t b = grp / nkv;
    const int64_t stride = DPART_HEAD + (int64_t)GT * h;
    const float* base = part + grp * splits * stride;
    const float c = scale * LOG2E;
    float M = -FLT_MAX;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, base[s * stride + R]);
    const int t = R / g;
    bf16_t* orow = out + (b * Tn + t) * ldo + ((int64_t)kvh * g + (R - t * g)) * h;
    for (int col = threadIdx.x; col < h; col += 256) {
        float num = 0.f, den = 0.f;
        for (int s = 0; s < nsplit; ++s) {
            const float* p = base + s * stride;
            const float ms = p[R];
            // a chunk in which the row saw nothing: the factor is the constant 0, no exp2 of a difference of sentinels
            const float w = ms == -FLT_MAX ? 0.f : __builtin_amdgcn_exp2f((ms - M) * c);
            den = __builtin_fmaf(w, p[DROWS + R], den);
            num = __builtin_fmaf(w, p[DPART_HEAD + (int64_t)R * h + col], num);
        }
        orow[col] = (bf16_t)(den > 0.f ? num / den : 0.f);
    }
}

// One workgroup per new row (b, t): the rotated q heads go to q_out, the rotated k heads and the v heads to row pos0 + t of the caches.
// AT: pos0 is *pos_d, in [0, max_pos] or every thread returns
template <class T, bool AT>
__global__ __launch_bounds__(256) void gemma_rope_cache_kernel(const T* __restrict__ qkv, int64_t ld_in, T* __restrict__ q_out, int64_t ldq,
                                                               T* __restrict__ kc, int64_t kbs, int64_t ldk, T* __restrict__ vc, int64_t vbs,
                                                               int64_t ldv, const float* __restrict__ table, int64_t rows, int Tn, int pos0, int nq,
                                                               int nkv, int h, const int32_t* __restrict__ pos_d, int max_pos) {
    if constexpr (AT) {
        pos0 = *pos_d;
        if (pos0 < 0 || pos0 > max_pos) return;
    }
    const int half = h / 2, pairs = (nq + nkv) * half, v_cols = nkv * h;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / Tn;
        const int64_t pos = pos0 + (row - b * Tn);
        const T* xr = qkv + row * ld_in;
        const float* tab = table + pos * h;
        T* qr = q_out + row * ldq;
        T* kr = kc + b * kbs + pos * ldk;
        T* vr = vc + b * vbs + pos * ldv;
        for (int p = threadIdx.x; p < pairs; p += 256) {
            const int head = p / half, i = p - head * half;
            const float sn = tab[i], cs = tab[half + i];
            const T* hx = xr + head * h;
            T* hy = head < nq ? qr + head * h : kr + (head - nq) * h;
            const float x1 = to_f32(hx[i]), x2 = to_f32(hx[half + i]);
            hy[2 * i] = from_f32<T>(__builtin_fmaf(x1, cs, -(x2 * sn)));
            hy[2 * i + 1] = from_f32<T>(__builtin_fmaf(x2, cs, x1 * sn));
        }
        for (int cidx = threadIdx.x; cidx < v_cols; cidx += 256) vr[cidx] = xr[(nq + nkv) * h + cidx];
    }
}

bool pitch_ok(int64_t ld, int64_t width) { return ld >= width && ld % 8 == 0; }

bool geometry_ok(int64_t batch, int pos0, int Tn, int nq, int nkv, int h) {
    return batch > 0 && pos0 >= 0 && Tn > 0 && (int64_t)pos0 + Tn <= INT_MAX - AK && nq > 0 && nkv > 0 && h > 0;
}

}  // namespace

#define GEMMA_UNSUPPORTED(cond, ...)          \
    do {                                      \
        if (!(cond)) {                        \
            iseg_set_error(__VA_ARGS__);      \
            return ISEG_ERR_UNSUPPORTED;      \
        }                                     \
    } while (0)

// both rope launchers: AT reads the position from pos_d when the kernel runs, pos0 is then unused
template <bool AT>
static int rope_cache_launch(const char* who, const void* qkv, int64_t ld_in, void* q_out, int64_t ldq, void* kcache, int64_t k_batch, int64_t ldk,
                             void* vcache, int64_t v_batch, int64_t ldv, const float* table, int64_t batch, int S, int pos0,
                             const int32_t* pos_d, int Tn, int nq, int nkv, int h, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(qkv && q_out && kcache && vcache && table && batch > 0 && S > 0 && Tn > 0 && nq > 0 && nkv > 0 && h > 0 && h % 2 == 0,
                 "%s: bad arguments", who);
    if constexpr (AT) {
        ISEG_REQUIRE(pos_d && (uintptr_t)pos_d % 4 == 0, "%s: the position is one aligned int32 in device memory", who);
        ISEG_REQUIRE(Tn <= S, "%s: %d new rows do not fit a cache of %d rows", who, Tn, S);
    } else {
        ISEG_REQUIRE(pos0 >= 0 && (int64_t)pos0 + Tn <= S, "%s: rows %d .. %lld do not lie inside a cache of %d rows", who, pos0,
                     (long long)pos0 + Tn - 1, S);
    }
    const int64_t width = (int64_t)(nq + 2 * nkv) * h;
    ISEG_REQUIRE(width <= INT_MAX && ld_in >= width && ldq >= (int64_t)nq * h && ldk >= (int64_t)nkv * h && ldv >= (int64_t)nkv * h &&
                     k_batch >= 0 && v_batch >= 0,
                 "%s: row pitches must cover their rows", who);
    const int64_t rows = batch * Tn;
    return by_dtype(dtype, who, [&](auto t) {
        using E = decltype(t);
        hipLaunchKernelGGL((gemma_rope_cache_kernel<E, AT>), dim3(grid_cap(rows, 1, 65536)), dim3(256), 0, stream, (const E*)qkv, ld_in, (E*)q_out,
                           ldq, (E*)kcache, k_batch, ldk, (E*)vcache, v_batch, ldv, table, rows, Tn, pos0, nq, nkv, h, pos_d, S - Tn);
        return iseg_check_launch(who);
    });
}

extern "C" int iseg_gemma_rope_cache(const void* qkv, int64_t ld_in, void* q_out, int64_t ldq, void* kcache, int64_t k_batch, int64_t ldk,
                                     void* vcache, int64_t v_batch, int64_t ldv, const float* table, int64_t batch, int S, int pos0, int Tn, int nq,
                                     int nkv, int h, int dtype, hipStream_t stream) {
    return rope_cache_launch<false>("iseg_gemma_rope_cache", qkv, ld_in, q_out, ldq, kcache, k_batch, ldk, vcache, v_batch, ldv, table, batch, S, pos0,
                                    nullptr, Tn, nq, nkv, h, dtype, stream);
}

extern "C" int iseg_gemma_rope_cache_at(const void* qkv, int64_t ld_in, void* q_out, int64_t ldq, void* kcache, int64_t k_batch, int64_t ldk,
                                        void* vcache, int64_t v_batch, int64_t ldv, const float* table, int64_t batch, int S, const int32_t* pos_d,
                                        int Tn, int nq, int nkv, int h, int dtype, hipStream_t stream) {
    return rope_cache_launch<true>("iseg_gemma_rope_cache_at", qkv, ld_in, q_out, ldq, kcache, k_batch, ldk, vcache, v_batch, ldv, table, batch, S, 0,
                                   pos_d, Tn, nq, nkv, h, dtype, stream);
}

extern "C" int iseg_gemma_decode_attention_supported(int Tn, int nq, int nkv, int h, int dtype) {
    return (dtype == ISEG_BF16 && h >= AD && h <= DH_MAX && h % AD == 0 && Tn > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 &&
            (int64_t)(nq / nkv) * Tn <= DROWS)
               ? 1
               : 0;
}

extern "C" int iseg_gemma_decode_attention_splits(int64_t batch, int pos0, int Tn, int nq, int nkv, int h) {
    if (!geometry_ok(batch, pos0, Tn, nq, nkv, h)) return 0;
    return plan_splits(batch, pos0, Tn, nkv);
}

extern "C" size_t iseg_gemma_decode_attention_scratch_bytes(int64_t batch, int pos0, int Tn, int nq, int nkv, int h, int splits) {
    if (!geometry_ok(batch, pos0, Tn, nq, nkv, h) || nq % nkv) return 0;
    const size_t partial = (size_t)DPART_HEAD + (size_t)(nq / nkv) * Tn * h;
    return (size_t)batch * nkv * resolve_splits(batch, pos0, Tn, nkv, splits) * partial * sizeof(float);
}

// both attention launchers.  AT: the position is read from pos_d when the kernels run; the grid and the workspace are planned for the
// capacity, pos0 = S - Tn, and `splits` travels to the kernels, which resolve it again for the position they find
template <bool AT>
static int decode_attention_launch(const char* who, const void* q, int64_t ldq, const void* kcache, int64_t k_batch, int64_t ldk, const void* vcache,
                                   int64_t v_batch, int64_t ldv, void* out, int64_t ldo, void* ws, size_t ws_bytes, int64_t batch, int S, int pos0,
                                   const int32_t* pos_d, int Tn, int nq, int nkv, int h, float scale, int splits, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(q && kcache && vcache && out && batch > 0 && S > 0 && Tn > 0, "%s: bad arguments", who);
    GEMMA_UNSUPPORTED(iseg_gemma_decode_attention_supported(Tn, nq, nkv, h, dtype),
                      "%s: needs bf16, a head width of 64, 128, 192 or 256, nq a multiple of nkv and (nq / nkv) * Tn <= 16 (got Tn %d, nq %d, nkv %d, h %d)",
                      who, Tn, nq, nkv, h);
    GEMMA_UNSUPPORTED(scale > 0.f && scale <= FLT_MAX, "%s: needs a positive finite scale", who);
    const int64_t wq = (int64_t)nq * h, wk = (int64_t)nkv * h;
    GEMMA_UNSUPPORTED(pitch_ok(ldq, wq) && pitch_ok(ldk, wk) && pitch_ok(ldv, wk) && pitch_ok(ldo, wq) && k_batch >= 0 && k_batch % 8 == 0 &&
                          v_batch >= 0 && v_batch % 8 == 0,
                      "%s: row pitches and batch strides must be multiples of 8 elements and the pitches cover their rows", who);
    GEMMA_UNSUPPORTED(((uintptr_t)q | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)out | (uintptr_t)ws) % 16 == 0,
                      "%s: operands must be 16-byte aligned", who);
    if constexpr (AT) {
        ISEG_REQUIRE(pos_d && (uintptr_t)pos_d % 4 == 0, "%s: the position is one aligned int32 in device memory", who);
        ISEG_REQUIRE(Tn <= S && S <= INT_MAX - AK, "%s: %d new rows do not fit a cache of %d rows", who, Tn, S);
        pos0 = S - Tn;
    } else {
        ISEG_REQUIRE(pos0 >= 0 && (int64_t)pos0 + Tn <= S && S <= INT_MAX - AK, "%s: rows %d .. %lld do not lie inside a cache of %d rows", who, pos0,
                     (long long)pos0 + Tn - 1, S);
    }
    const int g = nq / nkv, tiles = visible_tiles(pos0, Tn), nsplit = resolve_splits(batch, pos0, Tn, nkv, splits);
    const int64_t items = batch * nkv * nsplit, rows = batch * nkv * g * Tn;
    ISEG_REQUIRE(items <= INT_MAX && rows <= INT_MAX, "%s: too many work items", who);
    ISEG_NEED_WORKSPACE(who, ws, ws_bytes, iseg_gemma_decode_attention_scratch_bytes(batch, pos0, Tn, nq, nkv, h, nsplit));
    const bf16_t *qp = (const bf16_t*)q, *kp = (const bf16_t*)kcache, *vp = (const bf16_t*)vcache;
    float* part = (float*)ws;
#define DECODE_PASS1(SLABS)                                                                                                                         \
    hipLaunchKernelGGL((gemma_decode_partial_kernel<SLABS, AT>), dim3((unsigned)items), dim3(64 * SLABS), 0, stream, qp, ldq, kp, k_batch, ldk, vp,   \
                       v_batch, ldv, part, Tn, pos0, nkv, g, nsplit, tiles, scale, pos_d, S - Tn, batch, splits)
    switch (h / AD) {
        case 1: DECODE_PASS1(1); break;
        case 2: DECODE_PASS1(2); break;
        case 3: DECODE_PASS1(3); break;
        default: DECODE_PASS1(4); break;
    }
#undef DECODE_PASS1
    hipLaunchKernelGGL((gemma_decode_merge_kernel<AT>), dim3((unsigned)rows), dim3(256), 0, stream, part, (bf16_t*)out, ldo, Tn, nkv, g, h, nsplit, scale,
                       pos_d, S - Tn, batch, splits);
    return iseg_check_launch(who);
}

extern "C" int iseg_gemma_decode_attention(const void* q, int64_t ldq, const void* kcache, int64_t k_batch, int64_t ldk, const void* vcache,
                                           int64_t v_batch, int64_t ldv, void* out, int64_t ldo, void* ws, size_t ws_bytes, int64_t batch, int S,
                                           int pos0, int Tn, int nq, int nkv, int h, float scale, int splits, int dtype, hipStream_t stream) {
    return decode_attention_launch<false>("iseg_gemma_decode_attention", q, ldq, kcache, k_batch, ldk, vcache, v_batch, ldv, out, ldo, ws, ws_bytes,
                                          batch, S, pos0, nullptr, Tn, nq, nkv, h, scale, splits, dtype, stream);
}

extern "C" int iseg_gemma_decode_attention_at(const void* q, int64_t ldq, const void* kcache, int64_t k_batch, int64_t ldk, const void* vcache,
                                              int64_t v_batch, int64_t ldv, void* out, int64_t ldo, void* ws, size_t ws_bytes, int64_t batch, int S,
                                              const int32_t* pos_d, int Tn, int nq, int nkv, int h, float scale, int splits, int dtype,
                                              hipStream_t stream) {
    return decode_attention_launch<true>("iseg_gemma_decode_attention_at", q, ldq, kcache, k_batch, ldk, vcache, v_batch, ldv, out, ldo, ws, ws_bytes,
                                         batch, S, 0, pos_d, Tn, nq, nkv, h, scale, splits, dtype, stream);
}
