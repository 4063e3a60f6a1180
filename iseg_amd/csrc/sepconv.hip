// The activation=False unit of Xception (reference backbones/xception_common.py:14-78):
//
//   x -> relu -> depthwise 3 x 3 (stride s in {1, 2}, dilation d, TF 'same') = z -> BN(mean, rstd, gamma, beta) = u -> u W (1 x 1, [Cin][Cout])
//
// with the BN folded into the pointwise GEMM: a = gamma * rstd, c = beta - a * mean, W' = diag(a) W, b' = c^T W, v = z W' + b'.  Neither relu(x)
// nor u is written.  Kernels (storage fp32 or bf16, NHWC, eight consecutive channels = one 16-byte chunk, arithmetic fp32):
//
//   relu_dwconv3:  z = dw3x3(relu(x)); training statistics as fixed-order per-tile partials [part][2C] (sum z, sum z^2 of the STORED z) that a
//                  second launch sums in part order into iseg_bn_stats' packed message [sum | sum^2 | count].
//   fold:          W' in the layouts asked for ([Cout][Cin] for the K-contiguous forward product, [Cin][Cout] for the data gradient) in the
//                  GEMM's operand dtype, and b' fp32 -- one launch: 64 x 64 tiles transposed through LDS, and b' summed over k in a fixed order.
//   fold_bwd:      with G = z^T dV and S = colsum(dV):  dW += diag(a) G + c S^T,  dbeta_k = sum_o W_ko S_o,
//                  dgamma_k = rstd_k (sum_o W_ko G_ko - mean_k dbeta_k)  -> sums [dbeta | dgamma] (iseg_bn_bwd_reduce's layout), and the
//                  same values booked into the parameter gradients (+=) when given.
//   bnfold_dwconv3_relu_bwd:  D = dV W'^T = gamma rstd du; dz = D + alpha + beta' z (training statistics: beta' = -gamma rstd^2 dgamma / n,
//                  alpha = -gamma rstd dbeta / n - beta' mean; moving statistics: 0); dx = [x > 0] dw3x3^T(dz) gathered per INPUT pixel, and
//                  the depthwise weight gradient sum relu(x) dz per tap from the same gather (every (output pixel, tap) pair meets exactly one
//                  input pixel), as per-part partials [part][9C] summed in part order into dw (+=).
//
// Both depthwise kernels are spatial-tile kernels.  A workgroup owns a TH x TW pixel tile (output pixels forward, input pixels backward) of one
// sample and CG channel chunks, and walks `tstep` tiles down the image.  Per tile it stages the tile's window plus its halo in LDS once, as fp32:
// relu(x) forward, dz = D + alpha + beta' z backward (so D and z are read once per workgroup, not nine times through the caches), then every tap
// reads LDS.  Lanes are (chunk, pixel lane) with the chunk fastest, so a pixel's channels are one contiguous global access.  The tiling depends
// on the shape only, so every sum runs in an order fixed by the shape: no float atomics, bit-reproducible.
#include "common.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_TW = 16;                     // tile width (pixels)
constexpr int SC_MAX_PARTS = 1024;            // per-workgroup partial rows of the statistics / weight-gradient sums
constexpr int SC_LDS_REGION = 48 * 1024;      // bytes of the staged window

struct ScGeom {
    int N, H, W, C, Ho, Wo, s, d, pt, pl;
};

struct ScTile {
    int TH, TW, CG, nchunks, groups, tiles_h, tiles_w, tstep, hsteps, RH, RW;
};

int sc_same(int in, int s, int d, int* pad) {      // TF 'same' for a 3-tap window: (out size, pad before)
    const int out = (in + s - 1) / s;
    int total = (out - 1) * s + 2 * d + 1 - in;
    if (total < 0) total = 0;
    *pad = total / 2;
    return out;
}

ScGeom sc_geom(int N, int H, int W, int C, int s, int d) {
    ScGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C; g.s = s; g.d = d;
    g.Ho = sc_same(H, s, d, &g.pt);
    g.Wo = sc_same(W, s, d, &g.pl);
    return g;
}

// forward: tiles of output pixels, window = their input footprint; backward: tiles of input pixels, window = the output pixels their taps meet
ScTile sc_tile(const ScGeom& g, bool bwd) {
    ScTile t;
    t.TW = SC_TW;
    t.TH = (!bwd && g.s == 2) ? 4 : 8;
    if (bwd) {
        t.RH = (t.TH - 1 + 2 * g.d) / g.s + 2;
        t.RW = (t.TW - 1 + 2 * g.d) / g.s + 2;
    } else {
        t.RH = (t.TH - 1) * g.s + 2 * g.d + 1;
        t.RW = (t.TW - 1) * g.s + 2 * g.d + 1;
    }
    t.nchunks = g.C / 8;
    t.CG = 8;
    while (t.CG > 1 && (t.CG / 2 >= t.nchunks || t.RH * t.RW * t.CG * 32 > SC_LDS_REGION)) t.CG /= 2;
    t.groups = (t.nchunks + t.CG - 1) / t.CG;
    const int outH = bwd ? g.H : g.Ho, outW = bwd ? g.W : g.Wo;
    t.tiles_h = (outH + t.TH - 1) / t.TH;
    t.tiles_w = (outW + t.TW - 1) / t.TW;
    const int64_t cols = (int64_t)g.N * t.tiles_w;
    t.tstep = 1;
    while (t.tstep < t.tiles_h && cols * ((t.tiles_h + t.tstep - 1) / t.tstep) > SC_MAX_PARTS) t.tstep *= 2;
    t.hsteps = (t.tiles_h + t.tstep - 1) / t.tstep;
    return t;
}

int64_t sc_parts(const ScGeom& g, const ScTile& t) { return (int64_t)g.N * t.hsteps * t.tiles_w; }
size_t sc_lds_bytes(const ScTile& t) { return (size_t)t.RH * t.RW * t.CG * 8 * sizeof(float); }

bool sc_shape_ok(int N, int H, int W, int C, int s, int d) {
    if (!(N > 0 && N <= 65535 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && (s == 1 || s == 2) && d >= 1 && d <= 8 && (s == 1 || d == 1)))
        return false;
    const ScGeom g = sc_geom(N, H, W, C, s, d);
    return sc_lds_bytes(sc_tile(g, false)) <= SC_LDS_REGION && sc_lds_bytes(sc_tile(g, true)) <= SC_LDS_REGION;
}

bool sc_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define SC_UNSUPPORTED(what, N, H, W, C, s, d)                                                                                              \
    do {                                                                                                                                    \
        iseg_set_error("%s: unsupported shape N=%d H=%d W=%d C=%d stride=%d dilation=%d (C %% 8 == 0, stride 1 or 2, stride 2 only undilated, " \
                       "dilation <= 8, 16-byte aligned tensors)", what, N, H, W, C, s, d);                                                  \
        return ISEG_ERR_UNSUPPORTED;                                                                                                        \
    } while (0)

__device__ __forceinline__ int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the nine taps of the workgroup's CG chunks into LDS (zeros past C)
__device__ __forceinline__ void sc_stage_taps(const float* __restrict__ w, float* wsh, int C, int ch0, int width) {
    for (int i = threadIdx.x; i < 9 * width; i += SC_THREADS) {
        const int k = i / width, cc = i % width;
        wsh[i] = ch0 + cc < C ? w[(int64_t)k * C + ch0 + cc] : 0.f;
    }
}

// Sum `n` per-lane values over the pixel lanes of each chunk, in lane order, into dst[k * C + channel] (k < n): red is [SC_THREADS][9].
__device__ __forceinline__ void sc_lane_sums(float (*red)[9], const float (*v)[8], int n, int CG, int ch0, int C, float* dst) {
    const int lanes = SC_THREADS / CG;
    for (int k = 0; k < n; ++k) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = v[k][e];
        __syncthreads();
        if (threadIdx.x < CG * 8) {
            const int c = threadIdx.x / 8, e = threadIdx.x % 8;
            const int ch = ch0 + c * 8 + e;
            float sum = 0.f;
            for (int l = 0; l < lanes; ++l) sum += red[l * CG + c][e];
            if (ch < C) dst[(int64_t)k * C + ch] = sum;
        }
    }
}

// ---- forward: z = dw3x3(relu(x)), optional per-part statistics partials ---------------------------------------------------------------------
template <class T, bool STATS>
__global__ __launch_bounds__(SC_THREADS) void sc_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ z,
                                                            float* __restrict__ partials, float* __restrict__ count_out, ScGeom g, ScTile t) {
    extern __shared__ float4 sc_dyn[];
    float* win = reinterpret_cast<float*>(sc_dyn);
    __shared__ float wsh[9 * 64];
    __shared__ float red[SC_THREADS][9];
    const int CG = t.CG, C = g.C;
    const int c = threadIdx.x % CG, lane = threadIdx.x / CG, lanes = SC_THREADS / CG;
    const int tw_i = blockIdx.x % t.tiles_w, hs = blockIdx.x / t.tiles_w, n = blockIdx.y;
    const int chunk = blockIdx.z * CG + c, ch0 = blockIdx.z * CG * 8;
    const bool chunk_ok = chunk < t.nchunks;
    sc_stage_taps(w, wsh, C, ch0, CG * 8);
    float st[2][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) st[0][e] = st[1][e] = 0.f;
    const T* xn = x + (int64_t)n * g.H * g.W * C;
    const int wo0 = tw_i * t.TW;
    for (int ts = 0; ts < t.tstep; ++ts) {
        const int th_i = hs * t.tstep + ts;
        if (th_i >= t.tiles_h) break;
        const int ho0 = th_i * t.TH;
        const int hb = ho0 * g.s - g.pt, wb = wo0 * g.s - g.pl;
        __syncthreads();      // the previous tile's window (and the taps, the first time) are no longer read / are written
        for (int i = threadIdx.x; i < t.RH * t.RW * CG; i += SC_THREADS) {
            const int cc = i % CG, r = i / CG;
            const int h = hb + r / t.RW, ww = wb + r % t.RW;
            const int ck = blockIdx.z * CG + cc;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (ck < t.nchunks && h >= 0 && h < g.H && ww >= 0 && ww < g.W) {
                load8<T>(xn + ((int64_t)h * g.W + ww) * C + ck * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = relu_f32(v[e]);
            }
            float* dst = win + (size_t)i * 8;
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        if (!chunk_ok) continue;
        for (int px = lane; px < t.TH * t.TW; px += lanes) {
            const int ho = ho0 + px / t.TW, wo = wo0 + px % t.TW;
            if (ho >= g.Ho || wo >= g.Wo) continue;
            const int rb = (px / t.TW) * g.s, cb = (px % t.TW) * g.s;
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int r = (rb + (k / 3) * g.d) * t.RW + cb + (k % 3) * g.d;
                const float* src = win + ((size_t)r * CG + c) * 8;
                const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
                const float4 wa = *reinterpret_cast<const float4*>(&wsh[k * CG * 8 + c * 8]);
                const float4 wb4 = *reinterpret_cast<const float4*>(&wsh[k * CG * 8 + c * 8 + 4]);
                acc[0] = fmaf(a.x, wa.x, acc[0]); acc[1] = fmaf(a.y, wa.y, acc[1]);
                acc[2] = fmaf(a.z, wa.z, acc[2]); acc[3] = fmaf(a.w, wa.w, acc[3]);
                acc[4] = fmaf(b.x, wb4.x, acc[4]); acc[5] = fmaf(b.y, wb4.y, acc[5]);
                acc[6] = fmaf(b.z, wb4.z, acc[6]); acc[7] = fmaf(b.w, wb4.w, acc[7]);
            }
            float zr[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) zr[e] = to_f32(from_f32<T>(acc[e]));      // statistics of the stored z (what the GEMM reads)
            store8<T>(z + (((int64_t)n * g.Ho + ho) * g.Wo + wo) * C + chunk * 8, zr);
            if (STATS) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    st[0][e] += zr[e];
                    st[1][e] = fmaf(zr[e], zr[e], st[1][e]);
                }
            }
        }
    }
    if (!STATS) return;
    const int64_t part = ((int64_t)n * t.hsteps + hs) * t.tiles_w + tw_i;
    sc_lane_sums(red, st, 2, CG, ch0, C, partials + part * 2 * C);
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *count_out = (float)((int64_t)g.N * g.Ho * g.Wo);
}

// ---- fold: Wt [Cout][Cin] = (a W)^T, Wn [Cin][Cout] = a W (operand dtype), bias [Cout] = c^T W -------------------------------------------------
// One launch, two kinds of workgroup: the first `tiles` each scale and transpose one 64 x 64 tile of W through LDS; the rest each sum b' for 8
// columns, 32 k-lanes per column combined through LDS in lane order.
constexpr int SC_BIAS_COLS = 8;

template <class T>
__global__ __launch_bounds__(SC_THREADS) void sc_fold_kernel(const float* __restrict__ W, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ Wt,
                                                             T* __restrict__ Wn, float* __restrict__ bias, int Cin, int Cout, int tiles_o, int tiles) {
    __shared__ float tile[64][65];
    if ((int)blockIdx.x < tiles) {
        const int o0 = (blockIdx.x % tiles_o) * 64, k0 = (blockIdx.x / tiles_o) * 64;
        const int col = threadIdx.x % 64, lane_k = threadIdx.x / 64;
#pragma unroll 4
        for (int kk = lane_k; kk < 64; kk += 4) {
            const int k = k0 + kk, o = o0 + col;
            float v = 0.f;
            if (k < Cin && o < Cout) {
                v = gamma[k] * rstd[k] * W[(int64_t)k * Cout + o];
                if (Wn) Wn[(int64_t)k * Cout + o] = from_f32<T>(v);
            }
            tile[kk][col] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int oo = lane_k; oo < 64; oo += 4) {
            const int o = o0 + oo, k = k0 + col;
            if (Wt && o < Cout && k < Cin) Wt[(int64_t)o * Cin + k] = from_f32<T>(tile[col][oo]);
        }
        return;
    }
    const int col = threadIdx.x % SC_BIAS_COLS, lane_k = threadIdx.x / SC_BIAS_COLS;      // 32 k-lanes
    const int o = ((int)blockIdx.x - tiles) * SC_BIAS_COLS + col;
    float bsum = 0.f;
    if (o < Cout) {
#pragma unroll 4
        for (int k = lane_k; k < Cin; k += SC_THREADS / SC_BIAS_COLS) {
            const float a = gamma[k] * rstd[k];
            bsum = fmaf(beta[k] - a * mean[k], W[(int64_t)k * Cout + o], bsum);
        }
    }
    float* red = &tile[0][0];
    red[threadIdx.x] = bsum;
    __syncthreads();
    if (lane_k == 0 && o < Cout) {
        float t = 0.f;
        for (int l = 0; l < SC_THREADS / SC_BIAS_COLS; ++l) t += red[l * SC_BIAS_COLS + col];
        bias[o] = t;
    }
}

// ---- fold backward: one workgroup per input channel k ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void sc_fold_bwd_kernel(const float* __restrict__ G, const float* __restrict__ S, const float* __restrict__ W,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float* __restrict__ dW, float* __restrict__ sums, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta_out, int Cin, int Cout) {
    __shared__ float red[2][SC_THREADS / 64];
    const int k = blockIdx.x;
    const float a = gamma[k] * rstd[k];
    const float c = beta[k] - a * mean[k];
    float ws = 0.f, wg = 0.f;
    const int64_t row = (int64_t)k * Cout;
    for (int o = threadIdx.x; o < Cout; o += SC_THREADS) {
        const float gv = G[row + o], sv = S[o], wv = W[row + o];
        ws = fmaf(wv, sv, ws);
        wg = fmaf(wv, gv, wg);
        if (dW) dW[row + o] += fmaf(a, gv, c * sv);
    }
    ws = wave_sum(ws);
    wg = wave_sum(wg);
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = ws;
        red[1][wave] = wg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float dbeta = 0.f, wgs = 0.f;
        for (int i = 0; i < SC_THREADS / 64; ++i) {
            dbeta += red[0][i];
            wgs += red[1][i];
        }
        const float dg = rstd[k] * (wgs - mean[k] * dbeta);
        sums[k] = dbeta;
        sums[Cin + k] = dg;
        if (dbeta_out) dbeta_out[k] += dbeta;
        if (dgamma) dgamma[k] += dg;
    }
}

// ---- backward: dx = [x > 0] dw3x3^T(dz), per-part partials of dw; dz = D + alpha + beta' z staged in LDS with its halo --------------------
template <class T>
__global__ __launch_bounds__(SC_THREADS) void sc_bwd_kernel(const T* __restrict__ D, const T* __restrict__ z, const T* __restrict__ x,
                                                            const float* __restrict__ w, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ sums, float inv_n, int train,
                                                            T* __restrict__ dx, float* __restrict__ partials, ScGeom g, ScTile t) {
    extern __shared__ float4 sc_dyn[];
    float* win = reinterpret_cast<float*>(sc_dyn);
    __shared__ float wsh[9 * 64];
    __shared__ float coef[2][64];      // alpha, beta' of the workgroup's channels
    __shared__ float red[SC_THREADS][9];
    const int CG = t.CG, C = g.C;
    const int c = threadIdx.x % CG, lane = threadIdx.x / CG, lanes = SC_THREADS / CG;
    const int tw_i = blockIdx.x % t.tiles_w, hs = blockIdx.x / t.tiles_w, n = blockIdx.y;
    const int chunk = blockIdx.z * CG + c, ch0 = blockIdx.z * CG * 8;
    const bool chunk_ok = chunk < t.nchunks;
    sc_stage_taps(w, wsh, C, ch0, CG * 8);
    if (threadIdx.x < CG * 8) {
        const int ch = ch0 + threadIdx.x;
        float al = 0.f, bp = 0.f;
        if (train && ch < C) {
            const float gr = gamma[ch] * rstd[ch];
            bp = -gr * rstd[ch] * sums[C + ch] * inv_n;
            al = -gr * sums[ch] * inv_n - bp * mean[ch];
        }
        coef[0][threadIdx.x] = al;
        coef[1][threadIdx.x] = bp;
    }
    float dwacc[9][8];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) dwacc[k][e] = 0.f;
    const int64_t nbase_o = (int64_t)n * g.Ho * g.Wo, nbase_i = (int64_t)n * g.H * g.W;
    const int w0 = tw_i * t.TW;
    const int wo_lo = floordiv(w0 + g.pl - 2 * g.d, g.s);
    for (int ts = 0; ts < t.tstep; ++ts) {
        const int th_i = hs * t.tstep + ts;
        if (th_i >= t.tiles_h) break;
        const int h0 = th_i * t.TH;
        const int ho_lo = floordiv(h0 + g.pt - 2 * g.d, g.s);
        __syncthreads();
        for (int i = threadIdx.x; i < t.RH * t.RW * CG; i += SC_THREADS) {
            const int cc = i % CG, r = i / CG;
            const int ho = ho_lo + r / t.RW, wo = wo_lo + r % t.RW;
            const int ck = blockIdx.z * CG + cc;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (ck < t.nchunks && ho >= 0 && ho < g.Ho && wo >= 0 && wo < g.Wo) {
                const int64_t off = (nbase_o + (int64_t)ho * g.Wo + wo) * C + ck * 8;
                float dv[8], zv[8];
                load8<T>(D + off, dv);
                load8<T>(z + off, zv);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaf(coef[1][cc * 8 + e], zv[e], dv[e] + coef[0][cc * 8 + e]);
            }
            float* dst = win + (size_t)i * 8;
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        if (!chunk_ok) continue;
        for (int px = lane; px < t.TH * t.TW; px += lanes) {
            const int h = h0 + px / t.TW, ww = w0 + px % t.TW;
            if (h >= g.H || ww >= g.W) continue;
            const int64_t off = (nbase_i + (int64_t)h * g.W + ww) * C + chunk * 8;
            float xv[8], acc[8];
            load8<T>(x + off, xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[e] = 0.f;
                xv[e] = relu_f32(xv[e]);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int hh = h + g.pt - i * g.d;
                if (g.s == 2 && (hh & 1)) continue;
                const int rh = (g.s == 2 ? (hh >> 1) : hh) - ho_lo;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int wq = ww + g.pl - j * g.d;
                    if (g.s == 2 && (wq & 1)) continue;
                    const int rw = (g.s == 2 ? (wq >> 1) : wq) - wo_lo;
                    // a tap whose output pixel lies outside the map holds dz = 0 in the window: it adds nothing, and relu(x) * 0 must not turn
                    // a NaN or an infinity in x into a NaN of a weight-gradient tap that the reference never pairs it with
                    if ((unsigned)(rh + ho_lo) >= (unsigned)g.Ho || (unsigned)(rw + wo_lo) >= (unsigned)g.Wo) continue;
                    const float* src = win + (((size_t)rh * t.RW + rw) * CG + c) * 8;
                    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
                    const float dz[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    const float* wk = &wsh[(i * 3 + j) * CG * 8 + c * 8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        acc[e] = fmaf(wk[e], dz[e], acc[e]);
                        dwacc[i * 3 + j][e] = fmaf(xv[e], dz[e], dwacc[i * 3 + j][e]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = xv[e] > 0.f ? acc[e] : 0.f;
            store8<T>(dx + off, acc);
        }
    }
    const int64_t part = ((int64_t)n * t.hsteps + hs) * t.tiles_w + tw_i;
    sc_lane_sums(red, dwacc, 9, CG, ch0, C, partials + part * 9 * C);
}

}  // namespace

extern "C" int iseg_sepconv_supported(int N, int H, int W, int C, int stride, int dil, int dtype) {
    return sc_shape_ok(N, H, W, C, stride, dil) && (dtype == ISEG_F32 || dtype == ISEG_BF16) ? 1 : 0;
}

extern "C" size_t iseg_relu_dwconv3_stats_workspace_bytes(int N, int H, int W, int C, int stride, int dil) {
    if (!sc_shape_ok(N, H, W, C, stride, dil)) return 0;
    const ScGeom g = sc_geom(N, H, W, C, stride, dil);
    return (size_t)sc_parts(g, sc_tile(g, false)) * 2 * C * sizeof(float);
}

extern "C" int iseg_relu_dwconv3_stats(const void* x, const float* w, void* z, float* packed, int N, int H, int W, int C, int stride, int dil,
                                       int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && w && z, "iseg_relu_dwconv3_stats: null pointer");
    if (!sc_shape_ok(N, H, W, C, stride, dil) || !sc_aligned(x) || !sc_aligned(w) || !sc_aligned(z))
        SC_UNSUPPORTED("iseg_relu_dwconv3_stats", N, H, W, C, stride, dil);
    const ScGeom g = sc_geom(N, H, W, C, stride, dil);
    const ScTile t = sc_tile(g, false);
    const dim3 grid(t.tiles_w * t.hsteps, N, t.groups);
    const size_t lds = sc_lds_bytes(t);
    float* part = (float*)ws;
    if (packed) ISEG_NEED_WORKSPACE("iseg_relu_dwconv3_stats", ws, ws_bytes, iseg_relu_dwconv3_stats_workspace_bytes(N, H, W, C, stride, dil));
    const int rc = by_dtype(dtype, "iseg_relu_dwconv3_stats", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL((packed ? sc_fwd_kernel<T, true> : sc_fwd_kernel<T, false>), grid, dim3(SC_THREADS), lds, stream, (const T*)x, w, (T*)z,
                           packed ? part : nullptr, packed ? packed + 2 * C : nullptr, g, t);
    });
    if (rc != ISEG_OK) return rc;
    if (packed) launch_reduce_rows({.partials = part, .P = (int)sc_parts(g, t), .pstride = 2 * (int64_t)C, .n = 2 * (int64_t)C, .out0 = packed, .n0 = 2 * (int64_t)C}, stream);
    return iseg_check_launch("iseg_relu_dwconv3_stats");
}

extern "C" int iseg_sepconv_fold(const float* W, const float* mean, const float* rstd, const float* gamma, const float* beta, void* Wt, void* Wn,
                                 float* bias, int Cin, int Cout, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(W && mean && rstd && gamma && beta && (Wt || Wn) && bias, "iseg_sepconv_fold: null pointer");
    ISEG_REQUIRE(Cin > 0 && Cout > 0, "iseg_sepconv_fold: bad shape");
    const int tiles_o = (Cout + 63) / 64, tiles = tiles_o * ((Cin + 63) / 64);
    const dim3 grid(tiles + (Cout + SC_BIAS_COLS - 1) / SC_BIAS_COLS);
    return by_dtype(dtype, "iseg_sepconv_fold", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(sc_fold_kernel<T>, grid, dim3(SC_THREADS), 0, stream, W, mean, rstd, gamma, beta, (T*)Wt, (T*)Wn, bias, Cin, Cout, tiles_o,
                           tiles);
        return iseg_check_launch("iseg_sepconv_fold");
    });
}

extern "C" int iseg_sepconv_fold_bwd(const float* G, const float* S, const float* W, const float* mean, const float* rstd, const float* gamma,
                                     const float* beta, float* dW, float* sums, float* dgamma, float* dbeta, int Cin, int Cout, hipStream_t stream) {
    ISEG_REQUIRE(G && S && W && mean && rstd && gamma && beta && sums, "iseg_sepconv_fold_bwd: null pointer");
    ISEG_REQUIRE(Cin > 0 && Cout > 0, "iseg_sepconv_fold_bwd: bad shape");
    hipLaunchKernelGGL(sc_fold_bwd_kernel, dim3(Cin), dim3(SC_THREADS), 0, stream, G, S, W, mean, rstd, gamma, beta, dW, sums, dgamma, dbeta, Cin, Cout);
    return iseg_check_launch("iseg_sepconv_fold_bwd");
}


extern "C" size_t iseg_bnfold_dwconv3_relu_bwd_workspace_bytes(int N, int H, int W, int C, int stride, int dil) {
    if (!sc_shape_ok(N, H, W, C, stride, dil)) return 0;
    const ScGeom g = sc_geom(N, H, W, C, stride, dil);
    return (size_t)sc_parts(g, sc_tile(g, true)) * 9 * C * sizeof(float);
}

extern "C" int iseg_bnfold_dwconv3_relu_bwd(const void* D, const void* z, const void* x, const float* w, const float* mean, const float* rstd,
                                            const float* gamma, const float* sums, float inv_n, int train, void* dx, float* dw, int N, int H,
                                            int W, int C, int stride, int dil, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(D && z && x && w && dx && dw, "iseg_bnfold_dwconv3_relu_bwd: null pointer");
    ISEG_REQUIRE(!train || (mean && rstd && gamma && sums), "iseg_bnfold_dwconv3_relu_bwd: training statistics need mean, rstd, gamma, sums");
    if (!sc_shape_ok(N, H, W, C, stride, dil) || !sc_aligned(D) || !sc_aligned(z) || !sc_aligned(x) || !sc_aligned(w) ||
        !sc_aligned(dx))
        SC_UNSUPPORTED("iseg_bnfold_dwconv3_relu_bwd", N, H, W, C, stride, dil);
    ISEG_NEED_WORKSPACE("iseg_bnfold_dwconv3_relu_bwd", ws, ws_bytes, iseg_bnfold_dwconv3_relu_bwd_workspace_bytes(N, H, W, C, stride, dil));
    const ScGeom g = sc_geom(N, H, W, C, stride, dil);
    const ScTile t = sc_tile(g, true);
    const dim3 grid(t.tiles_w * t.hsteps, N, t.groups);
    const size_t lds = sc_lds_bytes(t);
    float* part = (float*)ws;
    const int rc = by_dtype(dtype, "iseg_bnfold_dwconv3_relu_bwd", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(sc_bwd_kernel<T>, grid, dim3(SC_THREADS), lds, stream, (const T*)D, (const T*)z, (const T*)x, w, mean, rstd, gamma, sums,
                           inv_n, train, (T*)dx, part, g, t);
    });
    if (rc != ISEG_OK) return rc;
    launch_reduce_rows({.partials = part, .P = (int)sc_parts(g, t), .pstride = 9 * (int64_t)C, .n = 9 * (int64_t)C, .out0 = dw, .n0 = 9 * (int64_t)C,
                        .accumulate = 1}, stream);
    return iseg_check_launch("iseg_bnfold_dwconv3_relu_bwd");
}
