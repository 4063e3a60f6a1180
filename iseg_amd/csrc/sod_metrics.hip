// Salient-object-detection metrics (metrics/sod/sod_metrics.py:114-1076 on metrics/sod/sod_metric_utils.py:17-229 of the reference): MAE,
// S-measure, E-measure (adaptive + 256-point curve), F-measure (adaptive + 257-point precision / recall / F curves) and the weighted
// F-measure, B images per call, each scored on its own, added to a caller-owned running state (fp64 sums, int64 count).
//
//   minmax   (normalize only) per-image min / max of the uint8 prediction, integer atomics                    sod_metric_utils.py:82-95
//   pass A   one read of pred + gt: fg / bg histograms of int(p * 255.0f), fg count, sum row*g, sum col*g, min / max of p over fg and bg
//            (integer atomics), and per-block fp64 partials of sum|p-g|, sum p, sum p / p^2 over fg, sum (1-p) / (1-p)^2 over bg
//   mid      thr = float(min(2 mean p, 1)), centroid (cy, cx) = rint(mean index) + 1 (round(h/2), round(w/2) + 1 for an empty foreground)
//   pass B   second read: counts of p >= thr and p >= thr && g, and per centroid quadrant sum p, sum p^2, sum p g (fp64 partials),
//            sum g and min / max of p (integer atomics)
//   wfm      column scan -> exact squared Euclidean distance + nearest foreground index per row -> Et = E[nearest] (kept as p[nearest])
//            -> 7x7 sigma=5 Gaussian on the foreground, min(E, EA), B = 2 - exp(ln(0.5)/5 Dst) on the background, weighted sums
//   finalize per image, fp64: every score and curve; then one launch adds the images to the running state in image order.
//
// Float sums are per-block partials added in a fixed order (lane -> wavefront butterfly -> four wavefronts -> blocks strided over 256 threads
// and a tree): bit-reproducible.  Only integers go through atomics.  Every accumulator is fp64: p is an fp32 value, so p * p, p - g and 1 - p
// are exact in fp64 and sum p^2 - N mean^2 cancels at 1e-16, not at 1e-7.  A region whose prediction is exactly constant (min == max, kept
// as integer atomics on the bit patterns) gets a variance of exactly 0, as exact arithmetic gives: the SSIM ladder of the reference
// (alpha == 0 && beta == 0 -> 1) is a discontinuity that a 1e-17 leftover would fall off.
//
// Histogram: saliency maps pile up in bins 0 and 255.  Each lane counts those four keys (fg / bg x 0 / 255) in registers, so they never
// reach LDS as atomics; the rest goes to the wavefront's own LDS copy of the histogram.  The four copies are merged once per workgroup and
// added to the image's histogram with one integer atomic per non-empty bin.
//
// Equidistant foreground pixels (weighted F-measure): the smallest row-major index wins.  scipy.ndimage.distance_transform_edt does not
// specify its choice; the two differ only where E differs between the tied candidates.
#include "common.h"
#include "iseg_hip.h"
#include "sod_common.h"

namespace {

constexpr int NI = ISEG_SOD_INTS;
constexpr int NS = ISEG_SOD_STATE_DOUBLES;
// the per-image integer record
constexpr int I_NFG = 512, I_NGE = 513, I_NGEFG = 514, I_CY = 515, I_CX = 516, I_THR = 517, I_UMIN = 518, I_UMAX = 519;
constexpr int I_FGMIN = 520, I_FGMAX = 521, I_BGMIN = 522, I_BGMAX = 523, I_QMIN = 524 /* [4][2]: min, max */, I_ROWSUM = 532, I_COLSUM = 534;
constexpr int I_QG = 536 /* [4] */;
// the state / per-image record of doubles
constexpr int S_MAE = 0, S_SM = 1, S_EM_ADP = 2, S_FM_ADP = 3, S_WFM = 4, S_EM = 5, S_FM = 261, S_PREC = 518, S_REC = 775;
constexpr int NPA = 6, NPB = 12, NPAB = NPA + NPB;
constexpr double D_EPS = 2.220446049250313e-16;      // EPS of sod_metric_utils.py:13 (2^-52 is an fp32 value too)
constexpr int NOMIN = 0x7fffffff;                    // a minimum is kept as max(NOMIN - bits): the record starts as zeros

__device__ __forceinline__ NormP norm_params(const int32_t* ir, int normalize) {
    return norm_from_minmax(255 - ir[I_UMIN], ir[I_UMAX], normalize);
}

// ---- minmax (normalize) -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sod_minmax_kernel(const uint8_t* __restrict__ pred, int64_t HW, int32_t* __restrict__ ints) {
    const int b = blockIdx.y;
    const uint8_t* p = pred + (int64_t)b * HW;
    int mx = 0, imn = 0;      // imn = 255 - min
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        const int u = p[i];
        mx = max(mx, u);
        imn = max(imn, 255 - u);
    }
    mx = wave_max_i(mx);
    imn = wave_max_i(imn);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(ints + (int64_t)b * NI + I_UMAX, mx);
        atomicMax(ints + (int64_t)b * NI + I_UMIN, imn);
    }
}

// ---- pass A --------------------------------------------------------------------------------------------------------------------------
struct AccA {
    double ad, sp, fp, fp2, bq, bq2;
    int nfg, c_b0, c_b255, c_f0, c_f255, fmin, fmax, bmin, bmax;
    unsigned long long rs, cs;
};

__device__ __forceinline__ void acc_a(AccA& a, float p, bool g, int row, int col, int* hist) {
    const double pd = (double)p;
    int bin = (int)(p * 255.0f);      // the fp32 product, truncated: sod_metrics.py:611 / :863
    bin = min(max(bin, 0), 255);
    const int bits = __float_as_int(fmaxf(p, 0.f));
    a.sp += pd;
    if (g) {
        a.ad += fabs(1.0 - pd);
        a.fp += pd;
        a.fp2 += pd * pd;
        a.nfg += 1;
        a.rs += (unsigned)row;
        a.cs += (unsigned)col;
        a.fmin = max(a.fmin, NOMIN - bits);
        a.fmax = max(a.fmax, bits);
        if (bin == 255) a.c_f255 += 1;
        else if (bin == 0) a.c_f0 += 1;
        else atomicAdd(hist + bin, 1);
    } else {
        const double q = 1.0 - pd;
        a.ad += fabs(pd);
        a.bq += q;
        a.bq2 += q * q;
        a.bmin = max(a.bmin, NOMIN - bits);
        a.bmax = max(a.bmax, bits);
        if (bin == 0) a.c_b0 += 1;
        else if (bin == 255) a.c_b255 += 1;
        else atomicAdd(hist + 256 + bin, 1);
    }
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(256) void sod_pass_a_kernel(const void* __restrict__ pred, const uint8_t* __restrict__ gt, int normalize, int H, int W,
                                                         int rpb, int bpi, int32_t* __restrict__ ints, double* __restrict__ part) {
    __shared__ int hist[4][512];
    __shared__ double red[4][NPA];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t* ir = ints + (int64_t)b * NI;
    for (int i = threadIdx.x; i < 4 * 512; i += 256) (&hist[0][0])[i] = 0;
    __syncthreads();
    const NormP np = norm_params(ir, normalize);
    const int gthr = normalize ? 128 : 0;
    const int64_t base = (int64_t)b * H * W;
    AccA a{};
    const int r1 = min(H, (blk + 1) * rpb);
    for (int r = blk * rpb + wid; r < r1; r += 4) {
        const int64_t ro = base + (int64_t)r * W;
        if (VEC) {
            for (int c = lane * 4; c < W; c += 256) {
                float p[4];
                bool g[4];
                load_p4<U8>(pred, ro + c, np, p);
                load_g4(gt, ro + c, gthr, g);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc_a(a, p[k], g[k], r, c + k, hist[wid]);
            }
        } else {
            for (int c = lane; c < W; c += 64) acc_a(a, load_p<U8>(pred, ro + c, np), gt[ro + c] > gthr, r, c, hist[wid]);
        }
    }
    // the four hot keys: one LDS add per wavefront
    const int h0 = wave_sum_i(a.c_b0), h1 = wave_sum_i(a.c_b255), h2 = wave_sum_i(a.c_f0), h3 = wave_sum_i(a.c_f255);
    if (lane == 0) {
        hist[wid][256] += h0;
        hist[wid][256 + 255] += h1;
        hist[wid][0] += h2;
        hist[wid][255] += h3;
    }
    const double v[NPA] = {a.ad, a.sp, a.fp, a.fp2, a.bq, a.bq2};
#pragma unroll
    for (int k = 0; k < NPA; ++k) {
        const double s = wave_sum_d(v[k]);
        if (lane == 0) red[wid][k] = s;
    }
    const int nfg = wave_sum_i(a.nfg);
    const unsigned long long rs = wave_sum_u64(a.rs), cs = wave_sum_u64(a.cs);
    const int fmin = wave_max_i(a.fmin), fmax = wave_max_i(a.fmax), bmin = wave_max_i(a.bmin), bmax = wave_max_i(a.bmax);
    if (lane == 0) {
        if (nfg) {
            atomicAdd(ir + I_NFG, nfg);
            atomicAdd(reinterpret_cast<unsigned long long*>(ir + I_ROWSUM), rs);
            atomicAdd(reinterpret_cast<unsigned long long*>(ir + I_COLSUM), cs);
        }
        atomicMax(ir + I_FGMIN, fmin);
        atomicMax(ir + I_FGMAX, fmax);
        atomicMax(ir + I_BGMIN, bmin);
        atomicMax(ir + I_BGMAX, bmax);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int s = (hist[0][i] + hist[1][i]) + (hist[2][i] + hist[3][i]);
        if (s) atomicAdd(ir + i, s);
    }
    if (threadIdx.x < NPA)
        part[((int64_t)b * bpi + blk) * NPAB + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- mid ---------------------------------------------------------------------------------------------------------------------------
// one wavefront per image: sum p over the blocks (lanes stride, butterfly), then lane 0 writes thr and the centroid
__global__ __launch_bounds__(64) void sod_mid_kernel(const double* __restrict__ part, int bpi, int H, int W, int32_t* __restrict__ ints) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double sp = 0.0;
    for (int t = lane; t < bpi; t += 64) sp += part[((int64_t)b * bpi + t) * NPAB + 1];
    sp = wave_sum_d(sp);
    if (lane == 0) {
        int32_t* ir = ints + (int64_t)b * NI;
        const double mean = sp / ((double)H * (double)W);
        const float thr = (float)fmin(2.0 * mean, 1.0);
        ir[I_THR] = __float_as_int(thr);
        const int nfg = ir[I_NFG];
        double cy, cx;
        if (nfg == 0) {
            cy = rint((double)H / 2.0);
            cx = rint((double)W / 2.0);
        } else {
            cy = rint((double)*reinterpret_cast<const unsigned long long*>(ir + I_ROWSUM) / (double)nfg);
            cx = rint((double)*reinterpret_cast<const unsigned long long*>(ir + I_COLSUM) / (double)nfg);
        }
        ir[I_CY] = (int)cy + 1;
        ir[I_CX] = (int)cx + 1;
    }
}

// ---- pass B ------------------------------------------------------------------------------------------------------------------------
struct AccQ {
    double sp, sp2, spg;
    int sg, mn, mx;
};

__device__ __forceinline__ void acc_q(AccQ& l, AccQ& r, bool left, float p, bool g) {
    const double pd = (double)p, p2 = pd * pd, pg = g ? pd : 0.0;
    const int bits = __float_as_int(fmaxf(p, 0.f));
    l.sp += left ? pd : 0.0;   r.sp += left ? 0.0 : pd;
    l.sp2 += left ? p2 : 0.0;  r.sp2 += left ? 0.0 : p2;
    l.spg += left ? pg : 0.0;  r.spg += left ? 0.0 : pg;
    l.sg += (left && g) ? 1 : 0;
    r.sg += (!left && g) ? 1 : 0;
    l.mn = max(l.mn, left ? NOMIN - bits : 0);  r.mn = max(r.mn, left ? 0 : NOMIN - bits);
    l.mx = max(l.mx, left ? bits : 0);          r.mx = max(r.mx, left ? 0 : bits);
}

// one image row of a wavefront: left of cx goes to L, the rest to R
template <bool U8, bool VEC>
__device__ __forceinline__ void row_b(const void* pred, const uint8_t* gt, int64_t ro, int W, int lane, int cx, float thr, int gthr, const NormP& np,
                                      AccQ& L, AccQ& R, int& nge, int& ngefg) {
    if (VEC) {
        for (int c = lane * 4; c < W; c += 256) {
            float p[4];
            bool g[4];
            load_p4<U8>(pred, ro + c, np, p);
            load_g4(gt, ro + c, gthr, g);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc_q(L, R, c + k < cx, p[k], g[k]);
                const bool ge = p[k] >= thr;
                nge += ge;
                ngefg += ge && g[k];
            }
        }
    } else {
        for (int c = lane; c < W; c += 64) {
            const float p = load_p<U8>(pred, ro + c, np);
            const bool g = gt[ro + c] > gthr;
            acc_q(L, R, c < cx, p, g);
            const bool ge = p >= thr;
            nge += ge;
            ngefg += ge && g;
        }
    }
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(256) void sod_pass_b_kernel(const void* __restrict__ pred, const uint8_t* __restrict__ gt, int normalize, int H, int W,
                                                         int rpb, int bpi, int32_t* __restrict__ ints, double* __restrict__ part) {
    __shared__ double red[4][NPB];
    const int b = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t* ir = ints + (int64_t)b * NI;
    const NormP np = norm_params(ir, normalize);
    const int gthr = normalize ? 128 : 0;
    const float thr = __int_as_float(ir[I_THR]);
    const int cy = ir[I_CY], cx = ir[I_CX];
    const int64_t base = (int64_t)b * H * W;
    AccQ q[4] = {};      // top-left, top-right, bottom-left, bottom-right
    int nge = 0, ngefg = 0;
    const int r1 = min(H, (blk + 1) * rpb);
    for (int r = blk * rpb + wid; r < r1; r += 4) {
        const int64_t ro = base + (int64_t)r * W;
        if (r < cy) row_b<U8, VEC>(pred, gt, ro, W, lane, cx, thr, gthr, np, q[0], q[1], nge, ngefg);      // the same branch for the whole wavefront
        else row_b<U8, VEC>(pred, gt, ro, W, lane, cx, thr, gthr, np, q[2], q[3], nge, ngefg);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s0 = wave_sum_d(q[k].sp), s1 = wave_sum_d(q[k].sp2), s2 = wave_sum_d(q[k].spg);
        const int sg = wave_sum_i(q[k].sg), mn = wave_max_i(q[k].mn), mx = wave_max_i(q[k].mx);
        if (lane == 0) {
            red[wid][k * 3 + 0] = s0;
            red[wid][k * 3 + 1] = s1;
            red[wid][k * 3 + 2] = s2;
            if (sg) atomicAdd(ir + I_QG + k, sg);
            atomicMax(ir + I_QMIN + 2 * k, mn);
            atomicMax(ir + I_QMIN + 2 * k + 1, mx);
        }
    }
    nge = wave_sum_i(nge);
    ngefg = wave_sum_i(ngefg);
    if (lane == 0) {
        if (nge) atomicAdd(ir + I_NGE, nge);
        if (ngefg) atomicAdd(ir + I_NGEFG, ngefg);
    }
    __syncthreads();
    if (threadIdx.x < NPB)
        part[((int64_t)b * bpi + blk) * NPAB + NPA + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- weighted F-measure ------------------------------------------------------------------------------------------------------------
// column scan: ny[y][x] = row of the nearest foreground pixel of column x (the upper one of two at the same distance), -1 for none.
// 64 columns x 16 row segments per workgroup: a wavefront first finds the first and last foreground row of its segment, the segments exchange
// them through LDS (the carry into a segment from above is the greatest "last" above it, from below the smallest "first" below it), and the
// wavefront then sweeps its segment down and up.  One thread per column over all H rows was a chain of 2 H dependent steps on 8 K threads.
constexpr int EDT_SEGS = 16;
__global__ __launch_bounds__(1024) void sod_edt_col_kernel(const uint8_t* __restrict__ gt, int gthr, int H, int W, const int32_t* __restrict__ ints,
                                                           int32_t* __restrict__ ny) {
    __shared__ int s_first[EDT_SEGS][64], s_last[EDT_SEGS][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, seg = threadIdx.x >> 6, x = blockIdx.x * 64 + lane;
    if (ints[(int64_t)b * NI + I_NFG] == 0) return;      // the whole workgroup
    const bool inx = x < W;
    const int rps = (H + EDT_SEGS - 1) / EDT_SEGS, y0 = seg * rps, y1 = min(H, y0 + rps);
    const uint8_t* g = gt + (int64_t)b * H * W + (inx ? x : 0);
    int32_t* o = ny + (int64_t)b * H * W + (inx ? x : 0);
    int first = -1, last = -1;
    if (inx)
        for (int y = y0; y < y1; ++y)
            if (g[(int64_t)y * W] > gthr) {
                if (first < 0) first = y;
                last = y;
            }
    s_first[seg][lane] = first;
    s_last[seg][lane] = last;
    __syncthreads();
    if (!inx) return;
    last = -1;
    for (int s2 = 0; s2 < seg; ++s2) last = max(last, s_last[s2][lane]);
    int next = -1;
    for (int s2 = EDT_SEGS - 1; s2 > seg; --s2)
        if (s_first[s2][lane] >= 0) next = s_first[s2][lane];
    for (int y = y0; y < y1; ++y) {
        if (g[(int64_t)y * W] > gthr) last = y;
        o[(int64_t)y * W] = last;
    }
    for (int y = y1 - 1; y >= y0; --y) {
        const int64_t i = (int64_t)y * W;
        if (g[i] > gthr) next = y;
        const int up = o[i];
        if (next >= 0 && (up < 0 || next - y < y - up)) o[i] = next;
    }
}

// one workgroup per row: d2[x] = min over x' of (x - x')^2 + (y - ny[x'])^2, scanning outward from x while dx^2 <= the best so far
template <bool U8>
__global__ __launch_bounds__(256) void sod_edt_row_kernel(const void* __restrict__ pred, int normalize, int H, int W, const int32_t* __restrict__ ints,
                                                          const int32_t* __restrict__ ny, int32_t* __restrict__ d2, int32_t* __restrict__ nearest,
                                                          float* __restrict__ Et) {
    extern __shared__ int s_row[];      // [W] squared vertical distance (-1: no foreground in the column), [W] its row
    int* s_g2 = s_row;
    int* s_ny = s_row + W;
    const int b = blockIdx.y, y = blockIdx.x;
    const int32_t* ir = ints + (int64_t)b * NI;
    if (ir[I_NFG] == 0) return;
    const NormP np = norm_params(ir, normalize);
    const int64_t base = (int64_t)b * H * W, ro = base + (int64_t)y * W;
    for (int x = threadIdx.x; x < W; x += 256) {
        const int n = ny[ro + x];
        s_ny[x] = n;
        s_g2[x] = n < 0 ? -1 : (y - n) * (y - n);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += 256) {
        int best = s_g2[x] < 0 ? NOMIN : s_g2[x];
        int bi = s_g2[x] < 0 ? NOMIN : s_ny[x] * W + x;
        const int reach = max(x, W - 1 - x);
        for (int dx = 1; dx <= reach; ++dx) {
            const int dx2 = dx * dx;
            if (dx2 > best) break;
            const int xl = x - dx, xr = x + dx;
            if (xl >= 0 && s_g2[xl] >= 0) {
                const int c = dx2 + s_g2[xl], idx = s_ny[xl] * W + xl;
                if (c < best || (c == best && idx < bi)) { best = c; bi = idx; }
            }
            if (xr < W && s_g2[xr] >= 0) {
                const int c = dx2 + s_g2[xr], idx = s_ny[xr] * W + xr;
                if (c < best || (c == best && idx < bi)) { best = c; bi = idx; }
            }
        }
        d2[ro + x] = best;
        if (nearest) nearest[ro + x] = bi;
        Et[ro + x] = load_p<U8>(pred, base + bi, np);      // p at the nearest foreground pixel (itself on the foreground): E = |p - 1| is formed in fp64
    }
}

struct Gauss7 {
    double k[49];
};

// 64 x 4 pixels per workgroup.  scipy.ndimage.convolve is a true convolution (flipped kernel); the Gaussian is symmetric, so the flip is moot.
template <bool U8>
__global__ __launch_bounds__(256) void sod_wfm_kernel(const void* __restrict__ pred, const uint8_t* __restrict__ gt, int normalize, int H, int W,
                                                      const int32_t* __restrict__ ints, const int32_t* __restrict__ d2, const float* __restrict__ Et,
                                                      Gauss7 K, double* __restrict__ part) {
    __shared__ double red[4][2];
    const int b = blockIdx.z, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int32_t* ir = ints + (int64_t)b * NI;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + wid;
    double efg = 0.0, ebg = 0.0;
    if (ir[I_NFG] != 0 && x < W && y < H) {
        const int64_t base = (int64_t)b * H * W, i = base + (int64_t)y * W + x;
        const bool g = gt[i] > (normalize ? 128 : 0);
        if (g) {
            double ea = 0.0;
#pragma unroll
            for (int dy = -3; dy <= 3; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
#pragma unroll
                for (int dx = -3; dx <= 3; ++dx) {
                    const int xx = x + dx;
                    if (xx >= 0 && xx < W) ea += K.k[(dy + 3) * 7 + dx + 3] * fabs(1.0 - (double)Et[base + (int64_t)yy * W + xx]);
                }
            }
            const double e = fabs(1.0 - (double)Et[i]);
            efg = ea < e ? ea : e;
        } else {
            const NormP np = norm_params(ir, normalize);
            const double e = (double)load_p<U8>(pred, i, np);
            const double dst = sqrt((double)d2[i]);
            ebg = e * (2.0 - exp(-0.13862943611198906 * dst));      // ln(0.5) / 5
        }
    }
    efg = wave_sum_d(efg);
    ebg = wave_sum_d(ebg);
    if (lane == 0) {
        red[wid][0] = efg;
        red[wid][1] = ebg;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int64_t nb = (int64_t)gridDim.x * gridDim.y;
        part[((int64_t)b * nb + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------
// sum of rec[t * stride] over t < n: 256 threads stride over the records, then a fixed tree; every thread gets the result
__device__ double block_sum_records(const double* rec, int64_t n, int stride, double* sm) {
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < n; t += 256) s += rec[t * stride];
    __syncthreads();
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    return sm[0];
}

// sod_metrics.py:539-597 / :599-713 for one threshold
__device__ double em_value(double ff, double fb, double nfg, double size) {
    const double pfg = ff + fb, pbg = size - pfg;
    double sum;
    if (nfg == 0.0) sum = pbg;
    else if (nfg == size) sum = pfg;
    else {
        const double bf = nfg - ff, bb = pbg - bf;
        const double mp = pfg / size, mg = nfg / size;
        const double dp[2] = {1.0 - mp, 0.0 - mp}, dg[2] = {1.0 - mg, 0.0 - mg};
        const double parts[4] = {ff, fb, bf, bb};
        sum = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = dp[k >> 1], c = dg[k & 1];
            const double al = 2.0 * (a * c) / (a * a + c * c + D_EPS);
            sum += ((al + 1.0) * (al + 1.0) / 4.0) * parts[k];
        }
    }
    return sum / (size - 1.0 + D_EPS);
}

// sod_metrics.py:274-286: 2 mean / (mean^2 + 1 + std + EPS), population std
__device__ double s_object(double s1, double s2, double n, bool constant) {
    const double mean = s1 / n;
    double var = s2 / n - mean * mean;
    if (constant || var < 0.0) var = 0.0;
    return 2.0 * mean / (mean * mean + 1.0 + sqrt(var) + D_EPS);
}

// sod_metrics.py:373-415.  N == 0: no pixels, contributes nothing (its weight is 0; the reference gives NaN).  N == 1: the variances of a
// single sample are taken as 0 (the reference divides 0 by 0), so the ladder gives 1 for alpha == beta == 0.
__device__ double ssim_q(double N, double sp, double sp2, double spg, double sg, bool p_const) {
    if (N <= 0.0) return 0.0;
    const double x = sp / N, y = sg / N;
    double sx = 0.0, sy = 0.0, sxy = 0.0;
    if (N > 1.0) {
        const bool g_const = sg == 0.0 || sg == N;
        sx = p_const ? 0.0 : (sp2 - N * x * x) / (N - 1.0);
        sy = g_const ? 0.0 : (sg - N * y * y) / (N - 1.0);
        sxy = (p_const || g_const) ? 0.0 : (spg - N * x * y) / (N - 1.0);
        if (sx < 0.0) sx = 0.0;
    }
    const double alpha = 4.0 * x * y * sxy, beta = (x * x + y * y) * (sx + sy);
    if (alpha != 0.0) return alpha / (beta + D_EPS);
    return beta == 0.0 ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void sod_finalize_kernel(const int32_t* __restrict__ ints, const double* __restrict__ part, int bpi,
                                                           const double* __restrict__ wpart, int64_t nw, int H, int W, int want_wfm, double alpha,
                                                           double beta, double beta_w, double* __restrict__ img) {
    __shared__ double sm[256];
    __shared__ double tot[NPAB + 2];
    __shared__ int hist[512];
    const int b = blockIdx.x, t = threadIdx.x;
    const int32_t* ir = ints + (int64_t)b * NI;
    double* o = img + (int64_t)b * NS;
    for (int k = 0; k < NPAB; ++k) {
        const double s = block_sum_records(part + (int64_t)b * bpi * NPAB + k, bpi, NPAB, sm);
        if (t == 0) tot[k] = s;
    }
    for (int k = 0; k < 2; ++k) {
        const double s = want_wfm ? block_sum_records(wpart + (int64_t)b * nw * 2 + k, nw, 2, sm) : 0.0;
        if (t == 0) tot[NPAB + k] = s;
    }
    hist[t] = ir[t];
    hist[256 + t] = ir[256 + t];
    __syncthreads();
    const double size = (double)H * (double)W, nfg = (double)ir[I_NFG];
    // index t of the 256-point curves is threshold 255 - t: everything in bins >= 255 - t
    double ff = 0.0, fb = 0.0;
    for (int k = 255 - t; k < 256; ++k) {
        ff += (double)hist[k];
        fb += (double)hist[256 + k];
    }
    o[S_EM + t] = em_value(ff, fb, nfg, size);
    // the 257-point curves: index i is threshold 256 - i; bin 256 is empty for p <= 1, so index 0 sees nothing and index i = t + 1 sees (ff, fb)
    {
        const double T = nfg > 1.0 ? nfg : 1.0;
        const double Ps = ff + fb;
        const double prec = Ps == 0.0 ? 0.0 : ff / Ps;
        const double rec = ff / T;
        const double num = (1.0 + beta) * prec * rec;
        const double den = num == 0.0 ? 1.0 : beta * prec + rec;
        o[S_PREC + t + 1] = prec;
        o[S_REC + t + 1] = rec;
        o[S_FM + t + 1] = num / den;
    }
    if (t == 0) {
        o[S_PREC] = 0.0;
        o[S_REC] = 0.0;
        o[S_FM] = 0.0;
        o[S_MAE] = tot[0] / size;
        // S-measure (sod_metrics.py:244-272)
        const double meanp = tot[1] / size;
        double sm_v;
        if (nfg == 0.0) sm_v = 1.0 - meanp;
        else if (nfg == size) sm_v = meanp;
        else {
            const double gm = nfg / size;
            const double obj = s_object(tot[2], tot[3], nfg, NOMIN - ir[I_FGMIN] == ir[I_FGMAX]) * gm +
                               s_object(tot[4], tot[5], size - nfg, NOMIN - ir[I_BGMIN] == ir[I_BGMAX]) * (1.0 - gm);
            const double cy = (double)ir[I_CY], cx = (double)ir[I_CX], h = (double)H, w = (double)W;
            const double w_lt = cy * cx / size, w_rt = cy * (w - cx) / size, w_lb = (h - cy) * cx / size;
            const double w_rb = 1.0 - w_lt - w_rt - w_lb;
            const double wq[4] = {w_lt, w_rt, w_lb, w_rb};
            const double nq[4] = {cy * cx, cy * (w - cx), (h - cy) * cx, (h - cy) * (w - cx)};
            double region = 0.0;
            for (int k = 0; k < 4; ++k) {
                const double* q = tot + NPA + 3 * k;
                const bool pc = NOMIN - ir[I_QMIN + 2 * k] == ir[I_QMIN + 2 * k + 1];
                if (nq[k] > 0.0) region += ssim_q(nq[k], q[0], q[1], q[2], (double)ir[I_QG + k], pc) * wq[k];
            }
            const double v = obj * alpha + region * (1.0 - alpha);
            sm_v = v > 0.0 ? v : 0.0;
        }
        o[S_SM] = sm_v;
        // adaptive E and F (sod_metrics.py:514-525, :821-851)
        const double nge = (double)ir[I_NGE], ngefg = (double)ir[I_NGEFG];
        o[S_EM_ADP] = em_value(ngefg, nge - ngefg, nfg, size);
        double fa = 0.0;
        if (ngefg != 0.0) {
            const double pre = ngefg / nge, rec = ngefg / nfg;
            fa = (1.0 + beta) * pre * rec / (beta * pre + rec);
        }
        o[S_FM_ADP] = fa;
        // weighted F (sod_metrics.py:1045-1053); 0 for an all-background gt (:989-993)
        double q = 0.0;
        if (want_wfm && nfg != 0.0) {
            const double efg = tot[NPAB], ebg = tot[NPAB + 1];
            const double TPw = nfg - efg, FPw = ebg;
            const double R = 1.0 - efg / nfg, P = TPw / (TPw + FPw + D_EPS);
            q = (1.0 + beta_w) * R * P / (R + beta_w * P + D_EPS);
        }
        o[S_WFM] = q;
    }
}

// state[j] += img[0][j] + img[1][j] + ... in image order; count += B
__global__ __launch_bounds__(256) void sod_accumulate_kernel(const double* __restrict__ img, int B, double* __restrict__ state, long long* __restrict__ count) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < NS) {
        double s = state[j];
        for (int b = 0; b < B; ++b) s += img[(int64_t)b * NS + j];
        state[j] = s;
    }
    if (j == 0) count[0] += B;
}

struct Layout {
    int rpb, bpi, wgx, wgy;
    int64_t nw, HW;
    size_t off_part, off_wpart, off_img, off_ny, off_d2, off_et, total;      // bytes
};

static inline Layout sod_layout(int B, int H, int W, int flags) {
    Layout l;
    // rows per workgroup from H alone (about 64 workgroups per image): the per-block partials of an image, and so the last bits of its scores,
    // must not depend on how many images share the call.  A workgroup's epilogue (wavefront reductions, a dozen integer atomics on the
    // image's record) is paid per workgroup, so rows are not spread thinner than that.
    int rpb = (H + 63) / 64;
    rpb = (rpb + 3) / 4 * 4;
    if (rpb < 4) rpb = 4;
    if (rpb > 64) rpb = 64;
    l.rpb = rpb;
    l.bpi = (H + rpb - 1) / rpb;
    l.wgx = (W + 63) / 64;
    l.wgy = (H + 3) / 4;
    l.nw = (int64_t)l.wgx * l.wgy;
    l.HW = (int64_t)H * W;
    const bool wfm = (flags & ISEG_SOD_WFM) != 0;
    size_t o = align256((size_t)B * NI * sizeof(int32_t));
    l.off_part = o;
    o += align256((size_t)B * l.bpi * NPAB * sizeof(double));
    l.off_wpart = o;
    o += wfm ? align256((size_t)B * l.nw * 2 * sizeof(double)) : 0;
    l.off_img = o;
    o += align256((size_t)B * NS * sizeof(double));
    l.off_ny = o;
    o += wfm ? align256((size_t)B * l.HW * 4) : 0;
    l.off_d2 = o;
    o += wfm ? align256((size_t)B * l.HW * 4) : 0;
    l.off_et = o;
    o += wfm ? align256((size_t)B * l.HW * 4) : 0;
    l.total = o;
    return l;
}

}  // namespace

extern "C" size_t iseg_sod_metrics_workspace_bytes(int B, int H, int W, int flags) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return sod_layout(B, H, W, flags).total;
}

extern "C" int iseg_sod_metrics(const void* pred, int pred_is_u8, const uint8_t* gt, int normalize, int B, int H, int W, int flags, double alpha,
                                double beta_fm, double beta_wfm, double* state, long long* count, int32_t* ints_out, double* per_image_out,
                                int32_t* dist2_out, int32_t* nearest_out, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(pred && gt && B > 0 && H > 0 && W > 0, "iseg_sod_metrics: bad arguments");
    ISEG_REQUIRE((pred_is_u8 != 0) == (normalize != 0), "iseg_sod_metrics: normalize takes a uint8 prediction, and only normalize does");
    ISEG_REQUIRE(H <= 16384 && W <= 16384, "iseg_sod_metrics: images beyond 16384 x 16384 are unsupported (32-bit squared distances)");
    ISEG_REQUIRE(B <= 65535, "iseg_sod_metrics: more than 65535 images per call");
    ISEG_REQUIRE(!(flags & ISEG_SOD_WFM) || W <= 8192, "iseg_sod_metrics: the weighted F-measure keeps one row of 2 W ints in 64 KiB of LDS: W <= 8192");
    ISEG_REQUIRE((state != nullptr) == (count != nullptr), "iseg_sod_metrics: state and count go together");
    const Layout l = sod_layout(B, H, W, flags);
    ISEG_NEED_WORKSPACE("iseg_sod_metrics", ws, ws_bytes, l.total);
    ISEG_REQUIRE_WORKSPACE(((uintptr_t)ws & 15) == 0, "iseg_sod_metrics: the workspace must be 16-byte aligned");
    const bool wfm = (flags & ISEG_SOD_WFM) != 0;
    ISEG_REQUIRE(wfm || (!dist2_out && !nearest_out), "iseg_sod_metrics: distances are only computed with ISEG_SOD_WFM");
    char* base = (char*)ws;
    int32_t* ints = (int32_t*)base;
    double* part = (double*)(base + l.off_part);
    double* wpart = (double*)(base + l.off_wpart);
    double* img = per_image_out ? per_image_out : (double*)(base + l.off_img);
    int32_t* ny = (int32_t*)(base + l.off_ny);
    int32_t* d2 = dist2_out ? dist2_out : (int32_t*)(base + l.off_d2);
    float* Et = (float*)(base + l.off_et);
    if (hipMemsetAsync(ints, 0, (size_t)B * NI * sizeof(int32_t), stream) != hipSuccess) {
        iseg_set_error("iseg_sod_metrics: hipMemsetAsync failed");
        return ISEG_ERR_HIP;
    }
    const bool u8 = pred_is_u8 != 0;
    const bool vec = W % 4 == 0 && ((uintptr_t)pred % 16 == 0) && ((uintptr_t)gt % 4 == 0);
    if (u8) {
        const int gx = (int)(ceil_div64(l.HW, 256 * 16) < 256 ? ceil_div64(l.HW, 256 * 16) : 256);
        hipLaunchKernelGGL(sod_minmax_kernel, dim3(gx, B), dim3(256), 0, stream, (const uint8_t*)pred, l.HW, ints);
    }
    const dim3 grid(l.bpi, B), block(256);
#define SOD_PASS(KERNEL, U, V) hipLaunchKernelGGL((KERNEL<U, V>), grid, block, 0, stream, pred, gt, normalize, H, W, l.rpb, l.bpi, ints, part)
#define SOD_PASSES(KERNEL)                        \
    do {                                          \
        if (u8 && vec) SOD_PASS(KERNEL, true, true);       \
        else if (u8) SOD_PASS(KERNEL, true, false);        \
        else if (vec) SOD_PASS(KERNEL, false, true);       \
        else SOD_PASS(KERNEL, false, false);               \
    } while (0)
    SOD_PASSES(sod_pass_a_kernel);
    hipLaunchKernelGGL(sod_mid_kernel, dim3(B), dim3(64), 0, stream, (const double*)part, l.bpi, H, W, ints);
    SOD_PASSES(sod_pass_b_kernel);
#undef SOD_PASSES
#undef SOD_PASS
    if (wfm) {
        // fspecial('gaussian', 7, 5) of sod_metric_utils.py:201-229 (no entry falls under EPS * max)
        Gauss7 K;
        double sum = 0.0;
        for (int y = -3; y <= 3; ++y)
            for (int x = -3; x <= 3; ++x) sum += K.k[(y + 3) * 7 + x + 3] = exp(-(double)(x * x + y * y) / 50.0);
        for (int i = 0; i < 49; ++i) K.k[i] /= sum;
        const int gthr = normalize ? 128 : 0;
        hipLaunchKernelGGL(sod_edt_col_kernel, dim3((W + 63) / 64, B), dim3(64 * EDT_SEGS), 0, stream, gt, gthr, H, W, (const int32_t*)ints, ny);
        const size_t lds = (size_t)W * 2 * sizeof(int);
        if (u8)
            hipLaunchKernelGGL((sod_edt_row_kernel<true>), dim3(H, B), dim3(256), lds, stream, pred, normalize, H, W, (const int32_t*)ints,
                               (const int32_t*)ny, d2, nearest_out, Et);
        else
            hipLaunchKernelGGL((sod_edt_row_kernel<false>), dim3(H, B), dim3(256), lds, stream, pred, normalize, H, W, (const int32_t*)ints,
                               (const int32_t*)ny, d2, nearest_out, Et);
        if (u8)
            hipLaunchKernelGGL((sod_wfm_kernel<true>), dim3(l.wgx, l.wgy, B), dim3(256), 0, stream, pred, gt, normalize, H, W, (const int32_t*)ints,
                               (const int32_t*)d2, (const float*)Et, K, wpart);
        else
            hipLaunchKernelGGL((sod_wfm_kernel<false>), dim3(l.wgx, l.wgy, B), dim3(256), 0, stream, pred, gt, normalize, H, W, (const int32_t*)ints,
                               (const int32_t*)d2, (const float*)Et, K, wpart);
    }
    hipLaunchKernelGGL(sod_finalize_kernel, dim3(B), dim3(256), 0, stream, (const int32_t*)ints, (const double*)part, l.bpi, (const double*)wpart,
                       l.nw, H, W, wfm ? 1 : 0, alpha, beta_fm, beta_wfm, img);
    if (state)
        hipLaunchKernelGGL(sod_accumulate_kernel, dim3((NS + 255) / 256), dim3(256), 0, stream, (const double*)img, B, state, count);
    if (ints_out &&
        hipMemcpyAsync(ints_out, ints, (size_t)B * NI * sizeof(int32_t), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        iseg_set_error("iseg_sod_metrics: hipMemcpyAsync failed");
        return ISEG_ERR_HIP;
    }
    return iseg_check_launch("iseg_sod_metrics");
}
