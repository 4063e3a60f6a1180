// Weighted, per-image confusion matrices from label / prediction maps: metrics/confusion_matrix.py:65-143 confusion_matrix and :146-231
// batch_confusion_matrix of the reference (tf.scatter_nd of the weights at [b, label, prediction]), and through them
// metrics/mean_iou.py:16-55 get_class_confusion_matrix / get_batch_class_confusion_matrix and :112-130 MeanIOU.update_state.
//
// Arithmetic: integers only, in every weight mode.  An element adds 1 (NONE), its weight byte (U8) or llrint((double)w * 2^w_exp) (F32: the
// power-of-two scale is exact in fp64, the rounding is to nearest even) to a 64-bit bin.  Integer sums do not depend on their order, so two runs,
// or any permutation of an image's pixels, give the same bits; there is no floating-point atomic in this file.
//
// Structure: a workgroup of 512 lanes belongs to ONE image at a time (blockIdx.y strides over the batch) and walks that image's slices of
// CM_SLICE = 4096 elements with a blockIdx.x stride; a lane reads two 16-byte chunks of each stream per slice (scalar dword loads when an image's
// row is not 16-byte aligned: n % 4 != 0).  Counts go to a workgroup-private histogram in LDS -- 32-bit bins for NONE / U8 (the launcher bounds
// the elements a workgroup can see per image so that 255 * elements < 2^32), 64-bit bins for F32 -- flushed once per image and band with 64-bit
// integer global atomics.  Where C * C bins exceed the 160 KiB of LDS the label rows are cut into `nbands` bands of `band_rows` rows and the
// index streams are walked once per band (an element is counted in the band its label falls in; the rejection counters are taken in band 0
// only).  The other route adds every element straight to the global matrix with integer atomics and needs no LDS.  The route table and the
// measurements behind it: DESIGN.md "Confusion matrices", profiles/confusion_kbench.md.
#include "common.h"
#include "iseg_hip.h"
#include <math.h>
#include <stdlib.h>

namespace {

constexpr int CM_THREADS = 512;
constexpr int CM_SLICE = ISEG_CM_SLICE;                  // Q: elements one workgroup consumes per trip = 512 lanes x 2 chunks x 4
constexpr int CM_GRID_CAP = ISEG_CM_GRID_CAP;            // workgroups per launch: 4 x 512 lanes on each of the 256 CUs
constexpr int CM_CUS = 256;
constexpr size_t CM_LDS_HEAD = 64;                       // six 64-bit rejection counters in front of the histogram
constexpr size_t CM_LDS_BYTES = 160 * 1024 - CM_LDS_HEAD;
constexpr int64_t CM_F32_MAX_N = ISEG_CM_F32_MAX_N;
constexpr int64_t CM_U32_MAX_ELEMS = 0xffffffffll / 255;      // 16 843 009 elements of weight 255 fit a 32-bit bin
constexpr int CM_MAX_BANDS = 4;                          // C = 256 with 64-bit bins: 4 bands of 64 rows

template <int WMODE> struct CmBin { using type = unsigned int; };
template <> struct CmBin<ISEG_CM_W_F32> { using type = unsigned long long; };
template <int WMODE> struct CmWeight { using type = unsigned char; };
template <> struct CmWeight<ISEG_CM_W_F32> { using type = float; };
constexpr int CM_LDS_MAX_BANDS = 4;                      // the route table: the LDS route up to this many bands, direct global atomics beyond

// four consecutive weights, 4-byte (U8) or 16-byte (F32) aligned
__device__ __forceinline__ void cm_load4(const unsigned char* p, unsigned char* out) {
    const unsigned int v = *reinterpret_cast<const unsigned int*>(p);
    out[0] = v & 255u, out[1] = (v >> 8) & 255u, out[2] = (v >> 16) & 255u, out[3] = v >> 24;
}
__device__ __forceinline__ void cm_load4(const float* p, float* out) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
}

struct CmArgs {
    const int32_t* labels;
    const int32_t* preds;
    const void* weights;
    double scale;            // 2^w_exp
    int64_t n, slices;
    int batch, C, use_ignore, ignore;
    long long* cm;
    unsigned long long* counters;
    int band_rows, nbands, use_lds;
};

// one element: the rules of include/iseg_hip.h, in their order
template <int WMODE, class BinT, class W>
__device__ __forceinline__ void cm_count(const CmArgs& a, int l, int p, W w, bool first_band, int r0, int r1, BinT* hist,
                                         unsigned long long* errs, unsigned long long* cmb, unsigned& inexact) {
    if (a.use_ignore && l == a.ignore) return;
    bool bad = false, frac = false;
    long long val = 1;
    if constexpr (WMODE == ISEG_CM_W_U8) val = (long long)w;
    if constexpr (WMODE == ISEG_CM_W_F32) {
        const double v = (double)w * a.scale;
        if (!(fabs(v) < 0x1p39)) {      // NaN, +-Inf and anything past the fixed-point range
            bad = true;
            if (first_band) atomicAdd(&errs[4], 1ull);
            val = 0;
        } else {
            const double r = rint(v);      // to nearest even
            val = (long long)r;
            frac = r != v;
        }
    }
    if (l < 0) { bad = true; if (first_band) atomicAdd(&errs[0], 1ull); }
    if (p < 0) { bad = true; if (first_band) atomicAdd(&errs[1], 1ull); }
    if (l >= a.C) { bad = true; if (first_band) atomicAdd(&errs[2], 1ull); }
    if (p >= a.C) { bad = true; if (first_band) atomicAdd(&errs[3], 1ull); }
    if (bad) return;
    if (frac && first_band) ++inexact;
    if (val == 0 || l < r0 || l >= r1) return;
    if (a.use_lds) atomicAdd(&hist[(l - r0) * a.C + p], (BinT)val);
    else atomicAdd(&cmb[(int64_t)l * a.C + p], (unsigned long long)val);      // (two's complement: a negative weight subtracts)
}

template <int WMODE, bool VEC>
__global__ __launch_bounds__(CM_THREADS) void confusion_kernel(CmArgs a) {
    using BinT = typename CmBin<WMODE>::type;
    using W = typename CmWeight<WMODE>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char cm_lds[];
    unsigned long long* errs = reinterpret_cast<unsigned long long*>(cm_lds);      // [6] (+ 2 unused)
    BinT* hist = reinterpret_cast<BinT*>(cm_lds + CM_LDS_HEAD);
    const int tid = threadIdx.x;
    for (int64_t b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const int32_t* lab = a.labels + b * a.n;
        const int32_t* prd = a.preds + b * a.n;
        const W* wts = WMODE == ISEG_CM_W_NONE ? nullptr : reinterpret_cast<const W*>(a.weights) + b * a.n;
        unsigned long long* cmb = reinterpret_cast<unsigned long long*>(a.cm) + b * (int64_t)a.C * a.C;
        if (tid < 8) errs[tid] = 0ull;
        unsigned inexact = 0u;      // at most n <= 2^24 per image in the one mode that counts it
        for (int band = 0; band < a.nbands; ++band) {
            const int r0 = band * a.band_rows, r1 = min(a.C, r0 + a.band_rows);
            const int nbins = (r1 - r0) * a.C;
            if (a.use_lds)
                for (int i = tid; i < nbins; i += CM_THREADS) hist[i] = 0;      // (the same lane read bin i in the last band's flush)
            __syncthreads();
            for (int64_t s = blockIdx.x; s < a.slices; s += gridDim.x) {
                const int64_t e0 = s * CM_SLICE;
                const int cnt = (int)(a.n - e0 < CM_SLICE ? a.n - e0 : CM_SLICE);
                if constexpr (VEC) {      // n % 4 == 0 and 16-byte aligned bases: cnt % 4 == 0, every chunk is whole
                    const int i0 = tid * 4, i1 = i0 + CM_THREADS * 4;
                    const bool h0 = i0 < cnt, h1 = i1 < cnt;
                    int4 l0 = {}, p0 = {}, l1 = {}, p1 = {};
                    W w0[4] = {}, w1[4] = {};
                    if (h0) {
                        l0 = *reinterpret_cast<const int4*>(lab + e0 + i0);
                        p0 = *reinterpret_cast<const int4*>(prd + e0 + i0);
                        if constexpr (WMODE != ISEG_CM_W_NONE) cm_load4(wts + e0 + i0, w0);
                    }
                    if (h1) {
                        l1 = *reinterpret_cast<const int4*>(lab + e0 + i1);
                        p1 = *reinterpret_cast<const int4*>(prd + e0 + i1);
                        if constexpr (WMODE != ISEG_CM_W_NONE) cm_load4(wts + e0 + i1, w1);
                    }
                    if (h0) {
                        cm_count<WMODE>(a, l0.x, p0.x, w0[0], band == 0, r0, r1, hist, errs, cmb, inexact);
                        cm_count<WMODE>(a, l0.y, p0.y, w0[1], band == 0, r0, r1, hist, errs, cmb, inexact);
                        cm_count<WMODE>(a, l0.z, p0.z, w0[2], band == 0, r0, r1, hist, errs, cmb, inexact);
                        cm_count<WMODE>(a, l0.w, p0.w, w0[3], band == 0, r0, r1, hist, errs, cmb, inexact);
                    }
                    if (h1) {
                        cm_count<WMODE>(a, l1.x, p1.x, w1[0], band == 0, r0, r1, hist, errs, cmb, inexact);
                        cm_count<WMODE>(a, l1.y, p1.y, w1[1], band == 0, r0, r1, hist, errs, cmb, inexact);
                        cm_count<WMODE>(a, l1.z, p1.z, w1[2], band == 0, r0, r1, hist, errs, cmb, inexact);
                        cm_count<WMODE>(a, l1.w, p1.w, w1[3], band == 0, r0, r1, hist, errs, cmb, inexact);
                    }
                } else {
                    for (int i = tid; i < cnt; i += CM_THREADS) {
                        W w = W(0);
                        if constexpr (WMODE != ISEG_CM_W_NONE) w = wts[e0 + i];
                        cm_count<WMODE>(a, lab[e0 + i], prd[e0 + i], w, band == 0, r0, r1, hist, errs, cmb, inexact);
                    }
                }
            }
            __syncthreads();
            if (a.use_lds)
                for (int i = tid; i < nbins; i += CM_THREADS) {
                    const BinT v = hist[i];
                    if (v) {
                        // a 64-bit bin holds a two's-complement sum; a 32-bit one a non-negative count
                        atomicAdd(&cmb[(int64_t)r0 * a.C + i], (unsigned long long)v);
                    }
                }
        }
        if (inexact) atomicAdd(&errs[5], (unsigned long long)inexact);
        __syncthreads();
        if (tid < 6 && errs[tid]) atomicAdd(&a.counters[tid], errs[tid]);
        __syncthreads();      // the next image clears errs
    }
}

// max over the bit patterns of |w|: for non-negative floats the integer order is the float order, so the integer maximum is exact and
// independent of the order; a NaN's pattern lies above +Inf's, so any non-finite weight shows as a pattern >= 0x7f800000
__global__ __launch_bounds__(256) void cm_absmax_kernel(const float* __restrict__ w, int64_t n, int vec, unsigned int* __restrict__ out) {
    unsigned int m = 0u;
    const int64_t stride = (int64_t)gridDim.x * 256, t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t j = t; j < n4; j += stride) {
        const uint4 v = *reinterpret_cast<const uint4*>(w + j * 4);
        m = max(max(m, v.x & 0x7fffffffu), max(v.y & 0x7fffffffu, max(v.z & 0x7fffffffu, v.w & 0x7fffffffu)));
    }
    for (int64_t j = n4 * 4 + t; j < n; j += stride) m = max(m, __float_as_uint(w[j]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// 0: by the table below; 1: the LDS route wherever its bands fit; 2: direct global atomics.  For tools/kbench_confusion.py, which measures
// the table's boundaries; the product never sets it.
int route_override() {
    static const int v = [] { const char* e = getenv("ISEG_CONFUSION_ROUTE"); return e ? atoi(e) : 0; }();
    return v;
}

template <int WMODE, bool VEC> int launch_confusion(const CmArgs& a, dim3 grid, size_t lds, hipStream_t stream) {
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&confusion_kernel<WMODE, VEC>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)(CM_LDS_BYTES + CM_LDS_HEAD)) == hipSuccess;
    if (!ok) {
        iseg_set_error("iseg_confusion_batched: cannot reserve %zu bytes of LDS", CM_LDS_BYTES + CM_LDS_HEAD);
        return ISEG_ERR_HIP;
    }
    hipLaunchKernelGGL((confusion_kernel<WMODE, VEC>), grid, dim3(CM_THREADS), lds, stream, a);
    return iseg_check_launch("iseg_confusion_batched");
}

}  // namespace

extern "C" int iseg_confusion_supported(int C, int wmode) {
    return C >= 1 && C <= 256 && wmode >= ISEG_CM_W_NONE && wmode <= ISEG_CM_W_F32;
}

extern "C" int iseg_confusion_absmax_f32(const float* w, int64_t n, uint32_t* max_bits, hipStream_t stream) {
    ISEG_REQUIRE(w && max_bits && n > 0, "iseg_confusion_absmax_f32: null pointer or n <= 0");
    if (hipMemsetAsync(max_bits, 0, sizeof(uint32_t), stream) != hipSuccess) return iseg_check_launch("iseg_confusion_absmax_f32");
    const int vec = ((uintptr_t)w & 15) == 0;
    hipLaunchKernelGGL(cm_absmax_kernel, dim3(grid_cap(n, 256 * 4, 1024)), dim3(256), 0, stream, w, n, vec, max_bits);
    return iseg_check_launch("iseg_confusion_absmax_f32");
}

extern "C" int iseg_confusion_batched(const int32_t* labels, const int32_t* preds, const void* weights, int wmode, int w_exp, int64_t batch,
                                      int64_t n, int C, int use_ignore, int ignore_label, long long* cm, int accumulate,
                                      unsigned long long* counters, hipStream_t stream) {
    ISEG_REQUIRE(labels && preds && cm && counters, "iseg_confusion_batched: null labels, preds, cm or counters");
    ISEG_REQUIRE(batch > 0 && n > 0, "iseg_confusion_batched: batch %lld and n %lld must be positive", (long long)batch, (long long)n);
    ISEG_REQUIRE(C >= 1 && C <= 256, "iseg_confusion_batched: C = %d outside 1..256", C);
    ISEG_REQUIRE(wmode >= ISEG_CM_W_NONE && wmode <= ISEG_CM_W_F32, "iseg_confusion_batched: unknown wmode %d", wmode);
    ISEG_REQUIRE(wmode == ISEG_CM_W_NONE || weights, "iseg_confusion_batched: wmode %d needs weights", wmode);
    ISEG_REQUIRE(batch <= 0x7fffffff && w_exp >= -1000 && w_exp <= 1000, "iseg_confusion_batched: batch %lld or w_exp %d out of range",
                 (long long)batch, w_exp);
    if (wmode == ISEG_CM_W_F32 && n > CM_F32_MAX_N) {
        iseg_set_error("iseg_confusion_batched: fp32 weights take n <= 2^24 elements per image (a bin stays below 2^62), got %lld", (long long)n);
        return ISEG_ERR_UNSUPPORTED;
    }
    // ---- route ----
    const size_t bin = wmode == ISEG_CM_W_F32 ? 8 : 4;
    int nbands = 1, band_rows = C;
    while (nbands <= CM_MAX_BANDS && (size_t)band_rows * C * bin > CM_LDS_BYTES) {
        ++nbands;
        band_rows = (C + nbands - 1) / nbands;
    }
    // (CM_MAX_BANDS = 4 covers C = 256 in 64-bit bins, so the LDS route exists for every supported C)
    int use_lds = nbands <= CM_LDS_MAX_BANDS;
    if (route_override() == 1) use_lds = nbands <= CM_MAX_BANDS;
    if (route_override() == 2) use_lds = 0;
    if (!use_lds) {
        nbands = 1;
        band_rows = C;
    }
    // ---- grid: gy images at a time, gx workgroups on the slices of each; no more workgroups than the CUs hold at once with this much LDS
    // (a workgroup that waits for a CU would zero and flush a histogram of its own: 1024 of them at C = 150 took 35 us on tiled maps where 256 take 24, profiles/confusion_kbench.md) ----
    const size_t lds = CM_LDS_HEAD + (use_lds ? (size_t)band_rows * C * bin : 0);
    const size_t per_cu = (CM_LDS_BYTES + CM_LDS_HEAD) / lds;
    const int cap = (int)(CM_CUS * per_cu < (size_t)CM_GRID_CAP ? CM_CUS * per_cu : (size_t)CM_GRID_CAP);      // at most four per CU
    const int64_t slices = ceil_div64(n, CM_SLICE);
    const unsigned gy = (unsigned)(batch < cap ? batch : cap);
    const unsigned gx = grid_cap(slices, 1, cap / gy);
    if (use_lds && bin == 4 && ceil_div64(slices, gx) * CM_SLICE > CM_U32_MAX_ELEMS) {
        iseg_set_error("iseg_confusion_batched: %lld elements per image on %u workgroups: more than %lld per workgroup would overflow its "
                       "32-bit counters", (long long)n, gx, (long long)CM_U32_MAX_ELEMS);
        return ISEG_ERR_UNSUPPORTED;
    }
    if (!accumulate && hipMemsetAsync(cm, 0, (size_t)batch * C * C * sizeof(long long), stream) != hipSuccess)
        return iseg_check_launch("iseg_confusion_batched");
    CmArgs a;
    a.labels = labels, a.preds = preds, a.weights = weights;
    a.scale = ldexp(1.0, w_exp);
    a.n = n, a.slices = slices;
    a.batch = (int)batch, a.C = C, a.use_ignore = use_ignore != 0, a.ignore = ignore_label;
    a.cm = cm, a.counters = counters;
    a.band_rows = band_rows, a.nbands = nbands, a.use_lds = use_lds;
    const dim3 grid(gx, gy);
    const bool vec = n % 4 == 0 && (((uintptr_t)labels | (uintptr_t)preds | (uintptr_t)weights) & 15) == 0;
    if (wmode == ISEG_CM_W_NONE) return vec ? launch_confusion<ISEG_CM_W_NONE, true>(a, grid, lds, stream) : launch_confusion<ISEG_CM_W_NONE, false>(a, grid, lds, stream);
    if (wmode == ISEG_CM_W_U8) return vec ? launch_confusion<ISEG_CM_W_U8, true>(a, grid, lds, stream) : launch_confusion<ISEG_CM_W_U8, false>(a, grid, lds, stream);
    return vec ? launch_confusion<ISEG_CM_W_F32, true>(a, grid, lds, stream) : launch_confusion<ISEG_CM_W_F32, false>(a, grid, lds, stream);
}
