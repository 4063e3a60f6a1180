// FmeasureV2 handlers (metrics/sod/fmeasurev2.py:117-237 and the compute_metric of :336-749 of the reference): IoU, specificity, Dice, overall
// accuracy, Kappa, precision, recall, FPR, BER and F-measure, each as a 256-point dynamic curve, at the adaptive threshold and at p > 0.5, B images
// per call, each scored on its own, added to a caller-owned running state ([n_handlers][264] fp64 sums, int64 count).  Everything a handler needs
// is four integers per threshold (TP, FP, TN, FN), so the streaming passes carry integer counters and one fp64 sum only.
//
//   uint8 + normalize
//     hist     ONE read of pred + gt: the 2 x 256 histogram of RAW grey levels by gt > 128 (integer atomics)
//     derive   one wavefront per image: min / max grey level, the 256 normalized fp32 values, their bins int(p * 255.0f), the fp64 mean
//              (sum of count * p: exact products), thr = float(min(2 mean, 1)), the p >= thr and p > 0.5 counts -- all from the 512 integers
//   fp32
//     pass 1   one read: fg / bg histograms of int(p * 255.0f), the p > 0.5 counts (integer atomics) and, for the adaptive mode, per-block
//              fp64 partials of sum p
//     mid      (adaptive mode only) thr = float(min(2 mean p, 1)), the partials summed in a fixed order
//     pass 2   (adaptive mode only) second read: counts of p >= thr and p >= thr && g
//   finalize one workgroup per image: suffix scan of both histograms -> TP[256], FP[256]; every handler's compute_metric in fp64 on the
//            exact integers (curve, adaptive, binary); then one launch adds the images to the running state in image order.
//
// Only integers go through atomics; the one float sum is per-block partials added in a fixed order (lane -> wavefront butterfly -> four
// wavefronts -> blocks strided over 64 lanes and a butterfly): bit-reproducible, and an image's partials depend on H * W alone, not on how many
// images share the call.  safe_divide's zero tests are made on the integer denominators.
//
// Histogram (fp32): saliency maps pile up in bins 0 and 255.  Each lane counts those four keys (fg / bg x 0 / 255) in registers, so they never
// reach LDS as atomics; the rest goes to the wavefront's own LDS copy of the histogram.  The four copies are merged once per workgroup and
// added to the image's histogram with one integer atomic per non-empty bin.
#include "common.h"
#include "iseg_hip.h"
#include "sod_common.h"

namespace {

constexpr int NI = ISEG_SODV2_INTS;
constexpr int ND = ISEG_SODV2_HANDLER_DOUBLES;
constexpr int MAXH = ISEG_SODV2_MAX_HANDLERS;
// the per-image integer record
constexpr int I_NFG = 512, I_NGE = 513, I_NGEFG = 514, I_N05 = 515, I_N05FG = 516, I_THR = 517;
// a handler's record of doubles
constexpr int D_ADP = 256, D_BIN = 257, D_BTP = 258;

struct Handlers {
    int n;
    int kind[MAXH];
    int mode[MAXH];
    double beta[MAXH];
};

__device__ __forceinline__ int bin_of(float p) {
    const int bin = (int)(p * 255.0f);      // the fp32 product, truncated: fmeasurev2.py:211
    return min(max(bin, 0), 255);
}

// ---- uint8: raw grey-level histogram ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void acc_raw4(unsigned pw, unsigned gw, int* hist) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned u = (pw >> (8 * k)) & 255u, g = (gw >> (8 * k)) & 255u;
        atomicAdd(hist + (g > 128u ? 0 : 256) + u, 1);
    }
}

// a workgroup owns `chunk` consecutive pixels of one image (chunk % 4096 == 0); VEC: 16 pixels per lane and load (HW % 16 == 0, aligned bases)
template <bool VEC>
__global__ __launch_bounds__(256) void fmv2_u8_hist_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t HW, int chunk,
                                                           int32_t* __restrict__ raw) {
    __shared__ int hist[4][512];
    const int b = blockIdx.y, wid = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 4 * 512; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const uint8_t* p = pred + (int64_t)b * HW;
    const uint8_t* g = gt + (int64_t)b * HW;
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(HW, i0 + chunk);
    if (VEC) {
        for (int64_t i = i0 + (int64_t)threadIdx.x * 16; i < i1; i += 256 * 16) {
            const uint4 pv = *reinterpret_cast<const uint4*>(p + i), gv = *reinterpret_cast<const uint4*>(g + i);
            acc_raw4(pv.x, gv.x, hist[wid]);
            acc_raw4(pv.y, gv.y, hist[wid]);
            acc_raw4(pv.z, gv.z, hist[wid]);
            acc_raw4(pv.w, gv.w, hist[wid]);
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) atomicAdd(hist[wid] + (g[i] > 128 ? 0 : 256) + p[i], 1);
    }
    __syncthreads();
    int32_t* rw = raw + (int64_t)b * 512;
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int s = (hist[0][i] + hist[1][i]) + (hist[2][i] + hist[3][i]);
        if (s) atomicAdd(rw + i, s);
    }
}

// one wavefront per image; lane l owns the grey levels l, l + 64, l + 128, l + 192
__global__ __launch_bounds__(64) void fmv2_u8_derive_kernel(const int32_t* __restrict__ raw, int64_t HW, int32_t* __restrict__ ints) {
    __shared__ int hist[512];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t* rw = raw + (int64_t)b * 512;
    int32_t* ir = ints + (int64_t)b * NI;
    for (int i = lane; i < 512; i += 64) hist[i] = 0;
    int cf[4], cb[4], mx = 0, imn = 0;      // imn = 255 - min
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int v = lane + 64 * k;
        cf[k] = rw[v];
        cb[k] = rw[256 + v];
        if (cf[k] + cb[k]) {
            mx = max(mx, v);
            imn = max(imn, 255 - v);
        }
    }
    mx = wave_max_i(mx);
    imn = wave_max_i(imn);
    const NormP np = norm_from_minmax(255 - imn, mx, 1);
    __syncthreads();
    float p[4];
    double sp = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k] = norm_u8(lane + 64 * k, np);
        const int bin = bin_of(p[k]);
        if (cf[k]) atomicAdd(hist + bin, cf[k]);
        if (cb[k]) atomicAdd(hist + 256 + bin, cb[k]);
        if (cf[k] + cb[k]) sp += (double)(cf[k] + cb[k]) * (double)p[k];      // exact: a count below 2^28 times an fp32 value
    }
    sp = wave_sum_d(sp);
    const float thr = (float)fmin(2.0 * (sp / (double)HW), 1.0);
    int nge = 0, ngefg = 0, n05 = 0, n05fg = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (cf[k] + cb[k] == 0) continue;
        if (p[k] >= thr) {
            nge += cf[k] + cb[k];
            ngefg += cf[k];
        }
        if (p[k] > 0.5f) {
            n05 += cf[k] + cb[k];
            n05fg += cf[k];
        }
    }
    nge = wave_sum_i(nge);
    ngefg = wave_sum_i(ngefg);
    n05 = wave_sum_i(n05);
    n05fg = wave_sum_i(n05fg);
    __syncthreads();
    for (int i = lane; i < 512; i += 64) ir[i] = hist[i];
    if (lane == 0) {
        ir[I_NGE] = nge;
        ir[I_NGEFG] = ngefg;
        ir[I_N05] = n05;
        ir[I_N05FG] = n05fg;
        ir[I_THR] = __float_as_int(thr);
    }
}

// ---- fp32: pass 1 --------------------------------------------------------------------------------------------------------------------
struct Acc1 {
    double sp;
    int c_b0, c_b255, c_f0, c_f255, n05, n05fg;
};

template <bool ADP> __device__ __forceinline__ void acc_1(Acc1& a, float p, bool g, int* hist) {
    const int bin = bin_of(p);
    const bool hi = p > 0.5f;
    if (ADP) a.sp += (double)p;
    a.n05 += hi;
    a.n05fg += hi && g;
    if (g) {
        if (bin == 255) a.c_f255 += 1;
        else if (bin == 0) a.c_f0 += 1;
        else atomicAdd(hist + bin, 1);
    } else {
        if (bin == 0) a.c_b0 += 1;
        else if (bin == 255) a.c_b255 += 1;
        else atomicAdd(hist + 256 + bin, 1);
    }
}

// a workgroup owns `chunk` consecutive pixels of one image (chunk % 4096 == 0); VEC: 4 pixels per lane and load (HW % 4 == 0, aligned bases)
template <bool VEC, bool ADP>
__global__ __launch_bounds__(256) void fmv2_pass1_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t HW, int chunk, int bpi,
                                                         int32_t* __restrict__ ints, double* __restrict__ part) {
    __shared__ int hist[4][512];
    __shared__ double red[4];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t* ir = ints + (int64_t)b * NI;
    for (int i = threadIdx.x; i < 4 * 512; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const float* p = pred + (int64_t)b * HW;
    const uint8_t* g = gt + (int64_t)b * HW;
    const int64_t i0 = (int64_t)blk * chunk, i1 = min(HW, i0 + chunk);
    Acc1 a{};
    const NormP id{0.f, 1.f, 0};
    if (VEC) {
        for (int64_t i = i0 + (int64_t)threadIdx.x * 4; i < i1; i += 1024) {
            float pv[4];
            bool gv[4];
            load_p4<false>(p, i, id, pv);
            load_g4(g, i, 0, gv);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc_1<ADP>(a, pv[k], gv[k], hist[wid]);
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) acc_1<ADP>(a, p[i], g[i] > 0, hist[wid]);
    }
    // the four hot keys: one LDS add per wavefront
    const int h0 = wave_sum_i(a.c_b0), h1 = wave_sum_i(a.c_b255), h2 = wave_sum_i(a.c_f0), h3 = wave_sum_i(a.c_f255);
    const int n05 = wave_sum_i(a.n05), n05fg = wave_sum_i(a.n05fg);
    if (lane == 0) {
        hist[wid][256] += h0;
        hist[wid][256 + 255] += h1;
        hist[wid][0] += h2;
        hist[wid][255] += h3;
        if (n05) atomicAdd(ir + I_N05, n05);
        if (n05fg) atomicAdd(ir + I_N05FG, n05fg);
    }
    if (ADP) {
        const double s = wave_sum_d(a.sp);
        if (lane == 0) red[wid] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int s = (hist[0][i] + hist[1][i]) + (hist[2][i] + hist[3][i]);
        if (s) atomicAdd(ir + i, s);
    }
    if (ADP && threadIdx.x == 0) part[(int64_t)b * bpi + blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one wavefront per image: sum p over the blocks (lanes stride, butterfly), then lane 0 writes thr
__global__ __launch_bounds__(64) void fmv2_mid_kernel(const double* __restrict__ part, int bpi, int64_t HW, int32_t* __restrict__ ints) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double sp = 0.0;
    for (int t = lane; t < bpi; t += 64) sp += part[(int64_t)b * bpi + t];
    sp = wave_sum_d(sp);
    if (lane == 0) ints[(int64_t)b * NI + I_THR] = __float_as_int((float)fmin(2.0 * (sp / (double)HW), 1.0));
}

// ---- fp32: pass 2 (adaptive mode) ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void fmv2_pass2_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t HW, int chunk,
                                                         int32_t* __restrict__ ints) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    int32_t* ir = ints + (int64_t)b * NI;
    const float thr = __int_as_float(ir[I_THR]);
    const float* p = pred + (int64_t)b * HW;
    const uint8_t* g = gt + (int64_t)b * HW;
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(HW, i0 + chunk);
    int nge = 0, ngefg = 0;
    const NormP id{0.f, 1.f, 0};
    if (VEC) {
        for (int64_t i = i0 + (int64_t)threadIdx.x * 4; i < i1; i += 1024) {
            float pv[4];
            bool gv[4];
            load_p4<false>(p, i, id, pv);
            load_g4(g, i, 0, gv);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ge = pv[k] >= thr;
                nge += ge;
                ngefg += ge && gv[k];
            }
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
            const bool ge = p[i] >= thr;
            nge += ge;
            ngefg += ge && g[i] > 0;
        }
    }
    nge = wave_sum_i(nge);
    ngefg = wave_sum_i(ngefg);
    if (lane == 0) {
        if (nge) atomicAdd(ir + I_NGE, nge);
        if (ngefg) atomicAdd(ir + I_NGEFG, ngefg);
    }
}

// ---- finalize ------------------------------------------------------------------------------------------------------------------------
// safe_divide (sod_metric_utils.py:138-152) with the zero test on the integer denominator
__device__ __forceinline__ double sdiv(double num, long long den) { return den == 0 ? 0.0 : num / (double)den; }

// compute_metric of fmeasurev2.py:336-749 on exact counts
__device__ double fmv2_metric(int kind, double beta, long long tp, long long fp, long long tn, long long fn) {
    switch (kind) {
    case ISEG_SODV2_IOU: return sdiv((double)tp, tp + fp + fn);
    case ISEG_SODV2_SPECIFICITY: return sdiv((double)tn, tn + fp);
    case ISEG_SODV2_DICE: return sdiv(2.0 * (double)tp, tp + fn + tp + fp);
    case ISEG_SODV2_OA: return sdiv((double)(tp + tn), tp + fp + tn + fn);
    case ISEG_SODV2_KAPPA: {
        // the reference's own formula (fmeasurev2.py:514-523): the second product is (tn + fn) * (tn + tp), as it writes it
        const long long total = tp + fp + tn + fn;
        const long long agree = (tp + fp) * (tp + fn) + (tn + fn) * (tn + tp), total2 = total * total;
        const double oa = sdiv((double)(tp + tn), total);
        const double hpy = sdiv((double)agree, total2);
        if (total2 != 0 && agree == total2) return 0.0;      // 1 - p_e == 0, tested on the integers
        const double d = 1.0 - hpy;      // rounds to 0 next to agree == total^2 only beyond 2^26 pixels
        return d == 0.0 ? 0.0 : (oa - hpy) / d;
    }
    case ISEG_SODV2_PRECISION: return sdiv((double)tp, tp + fp);
    case ISEG_SODV2_RECALL: return sdiv((double)tp, tp + fn);
    case ISEG_SODV2_FPR: return sdiv((double)fp, tn + fp);
    case ISEG_SODV2_BER: return 1.0 - 0.5 * (sdiv((double)tp, tp + fn) + sdiv((double)tn, tn + fp));
    default: {      // ISEG_SODV2_FMEASURE
        const double pre = sdiv((double)tp, tp + fp), rec = sdiv((double)tp, tp + fn);
        const double den = beta * pre + rec;
        return den == 0.0 ? 0.0 : (beta + 1.0) * pre * rec / den;
    }
    }
}

// inclusive scan of s[0..255] over 256 threads
__device__ __forceinline__ void block_scan_256(int* s) {
    const int t = threadIdx.x;
    for (int o = 1; o < 256; o <<= 1) {
        const int v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fmv2_finalize_kernel(int32_t* __restrict__ ints, int64_t HW, Handlers hs, double* __restrict__ img) {
    __shared__ int s_tp[256], s_fp[256];
    const int b = blockIdx.x, t = threadIdx.x;
    int32_t* ir = ints + (int64_t)b * NI;
    // index t of the curve is threshold 255 - t: everything in bins >= 255 - t (cumsum of the reversed histogram, fmeasurev2.py:229-230)
    s_tp[t] = ir[255 - t];
    s_fp[t] = ir[256 + 255 - t];
    __syncthreads();
    block_scan_256(s_tp);
    block_scan_256(s_fp);
    const long long FG = s_tp[255], BG = HW - FG;
    if (t == 0) ir[I_NFG] = (int)FG;
    const long long tp = s_tp[t], fp = s_fp[t];
    const long long atp = ir[I_NGEFG], afp = ir[I_NGE] - ir[I_NGEFG], btp = ir[I_N05FG], bfp = ir[I_N05] - ir[I_N05FG];
    for (int h = 0; h < hs.n; ++h) {
        const int kind = hs.kind[h], mode = hs.mode[h];
        const double beta = hs.beta[h];
        double* o = img + ((int64_t)b * hs.n + h) * ND;
        o[t] = (mode & ISEG_SODV2_DYNAMIC) ? fmv2_metric(kind, beta, tp, fp, BG - fp, FG - tp) : 0.0;
        if (t < ND - 256) {
            double v = 0.0;
            if (t == 0 && (mode & ISEG_SODV2_ADAPTIVE)) v = fmv2_metric(kind, beta, atp, afp, BG - afp, FG - atp);
            if (t >= 1 && (mode & ISEG_SODV2_BINARY)) {
                if (t == 1) v = fmv2_metric(kind, beta, btp, bfp, BG - bfp, FG - btp);
                else if (t == 2) v = (double)btp;
                else if (t == 3) v = (double)bfp;
                else if (t == 4) v = (double)(BG - bfp);
                else if (t == 5) v = (double)(FG - btp);
            }
            o[256 + t] = v;
        }
    }
}

// state[j] += img[0][j] + img[1][j] + ... in image order; count += B
__global__ __launch_bounds__(256) void fmv2_accumulate_kernel(const double* __restrict__ img, int B, int n, double* __restrict__ state,
                                                              long long* __restrict__ count) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) {
        double s = state[j];
        for (int b = 0; b < B; ++b) s += img[(int64_t)b * n + j];
        state[j] = s;
    }
    if (j == 0) count[0] += B;
}

struct Layout {
    int chunk, bpi;
    int64_t HW;
    size_t off_raw, off_part, off_img, total;      // bytes
};

static inline Layout fmv2_layout(int B, int H, int W, int n_handlers) {
    Layout l;
    l.HW = (int64_t)H * W;
    // pixels per workgroup from H * W alone (about 64 workgroups per image, 4 Ki to 64 Ki pixels each): the per-block partials of an image, and so
    // the last bit of its threshold, must not depend on how many images share the call
    int64_t chunk = ceil_div64(ceil_div64(l.HW, 64), 4096) * 4096;
    if (chunk > 65536) chunk = 65536;
    l.chunk = (int)chunk;
    l.bpi = (int)ceil_div64(l.HW, chunk);
    size_t o = align256((size_t)B * NI * sizeof(int32_t));
    l.off_raw = o;
    o += align256((size_t)B * 512 * sizeof(int32_t));
    l.off_part = o;
    o += align256((size_t)B * l.bpi * sizeof(double));
    l.off_img = o;
    o += align256((size_t)B * n_handlers * ND * sizeof(double));
    l.total = o;
    return l;
}

}  // namespace

extern "C" size_t iseg_sod_fmv2_workspace_bytes(int B, int H, int W, int n_handlers) {
    if (B <= 0 || H <= 0 || W <= 0 || n_handlers <= 0 || n_handlers > MAXH) return 0;
    return fmv2_layout(B, H, W, n_handlers).total;
}

extern "C" int iseg_sod_fmv2(const void* pred, int pred_is_u8, const uint8_t* gt, int normalize, int B, int H, int W, int n_handlers,
                             const int32_t* kinds_h, const int32_t* modes_h, const double* betas_h, double* state, long long* count,
                             int32_t* ints_out, double* per_image_out, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(pred && gt && B > 0 && H > 0 && W > 0, "iseg_sod_fmv2: bad arguments");
    ISEG_REQUIRE((pred_is_u8 != 0) == (normalize != 0), "iseg_sod_fmv2: normalize takes a uint8 prediction, and only normalize does");
    ISEG_REQUIRE(H <= 16384 && W <= 16384, "iseg_sod_fmv2: images beyond 16384 x 16384 are unsupported (32-bit counts)");
    ISEG_REQUIRE(B <= 65535, "iseg_sod_fmv2: more than 65535 images per call");
    ISEG_REQUIRE(n_handlers >= 1 && n_handlers <= MAXH, "iseg_sod_fmv2: %d handlers (1..%d)", n_handlers, MAXH);
    ISEG_REQUIRE(kinds_h && modes_h && betas_h, "iseg_sod_fmv2: the handler tables are host arrays of n_handlers entries");
    ISEG_REQUIRE((state != nullptr) == (count != nullptr), "iseg_sod_fmv2: state and count go together");
    Handlers hs{};
    hs.n = n_handlers;
    int modes = 0;
    for (int h = 0; h < n_handlers; ++h) {
        ISEG_REQUIRE(kinds_h[h] >= ISEG_SODV2_IOU && kinds_h[h] <= ISEG_SODV2_FMEASURE, "iseg_sod_fmv2: handler %d has the unknown kind %d", h, kinds_h[h]);
        ISEG_REQUIRE((modes_h[h] & ~(ISEG_SODV2_DYNAMIC | ISEG_SODV2_ADAPTIVE | ISEG_SODV2_BINARY)) == 0, "iseg_sod_fmv2: handler %d has the unknown mode bits %d",
                     h, modes_h[h]);
        hs.kind[h] = kinds_h[h];
        hs.mode[h] = modes_h[h];
        hs.beta[h] = betas_h[h];
        modes |= modes_h[h];
    }
    const Layout l = fmv2_layout(B, H, W, n_handlers);
    ISEG_NEED_WORKSPACE("iseg_sod_fmv2", ws, ws_bytes, l.total);
    ISEG_REQUIRE_WORKSPACE(((uintptr_t)ws & 15) == 0, "iseg_sod_fmv2: the workspace must be 16-byte aligned");
    char* base = (char*)ws;
    int32_t* ints = (int32_t*)base;
    int32_t* raw = (int32_t*)(base + l.off_raw);
    double* part = (double*)(base + l.off_part);
    double* img = per_image_out ? per_image_out : (double*)(base + l.off_img);
    const bool u8 = pred_is_u8 != 0;
    // the integer records and, behind them, the raw grey-level histograms
    if (hipMemsetAsync(ints, 0, u8 ? l.off_part : l.off_raw, stream) != hipSuccess) {
        iseg_set_error("iseg_sod_fmv2: hipMemsetAsync failed");
        return ISEG_ERR_HIP;
    }
    const dim3 grid(l.bpi, B), block(256);
    if (u8) {
        const bool vec = l.HW % 16 == 0 && ((uintptr_t)pred % 16 == 0) && ((uintptr_t)gt % 16 == 0);
        if (vec) hipLaunchKernelGGL((fmv2_u8_hist_kernel<true>), grid, block, 0, stream, (const uint8_t*)pred, gt, l.HW, l.chunk, raw);
        else hipLaunchKernelGGL((fmv2_u8_hist_kernel<false>), grid, block, 0, stream, (const uint8_t*)pred, gt, l.HW, l.chunk, raw);
        hipLaunchKernelGGL(fmv2_u8_derive_kernel, dim3(B), dim3(64), 0, stream, (const int32_t*)raw, l.HW, ints);
    } else {
        const float* pf = (const float*)pred;
        const bool vec = l.HW % 4 == 0 && ((uintptr_t)pred % 16 == 0) && ((uintptr_t)gt % 4 == 0);
        const bool adp = (modes & ISEG_SODV2_ADAPTIVE) != 0;
#define FMV2_PASS1(V, A) hipLaunchKernelGGL((fmv2_pass1_kernel<V, A>), grid, block, 0, stream, pf, gt, l.HW, l.chunk, l.bpi, ints, part)
        if (vec && adp) FMV2_PASS1(true, true);
        else if (vec) FMV2_PASS1(true, false);
        else if (adp) FMV2_PASS1(false, true);
        else FMV2_PASS1(false, false);
#undef FMV2_PASS1
        if (adp) {
            hipLaunchKernelGGL(fmv2_mid_kernel, dim3(B), dim3(64), 0, stream, (const double*)part, l.bpi, l.HW, ints);
            if (vec) hipLaunchKernelGGL((fmv2_pass2_kernel<true>), grid, block, 0, stream, pf, gt, l.HW, l.chunk, ints);
            else hipLaunchKernelGGL((fmv2_pass2_kernel<false>), grid, block, 0, stream, pf, gt, l.HW, l.chunk, ints);
        }
    }
    hipLaunchKernelGGL(fmv2_finalize_kernel, dim3(B), dim3(256), 0, stream, ints, l.HW, hs, img);
    if (state) {
        const int n = n_handlers * ND;
        hipLaunchKernelGGL(fmv2_accumulate_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const double*)img, B, n, state, count);
    }
    if (ints_out &&
        hipMemcpyAsync(ints_out, ints, (size_t)B * NI * sizeof(int32_t), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        iseg_set_error("iseg_sod_fmv2: hipMemcpyAsync failed");
        return ISEG_ERR_HIP;
    }
    return iseg_check_launch("iseg_sod_fmv2");
}
