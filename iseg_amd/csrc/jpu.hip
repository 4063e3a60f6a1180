// The tail of JointPyramidUpsampling (reference layers/jpu.py:38-59, 79-88): one merged map through four separable branches
//
//   x -> depthwise 3 x 3 (dilation r, TF 'same', WITH bias) = z_r -> BN_r(mean, rstd, gamma, beta) = u_r -> u_r W_r (1 x 1),   r = 1, 2, 4, 8
//
// Every BN is folded into its pointwise GEMM exactly as csrc/sepconv.hip does it (a = gamma * rstd, c = beta - a * mean, W' = diag(a) W,
// b' = c^T W, v = z W' + b'; fold and fold_bwd are sepconv.hip's), so the depthwise side is all that is new here.  The rates are compile-time
// constants, the stride is 1, and 'same' is a pad of r on each side.  Storage fp32 or bf16, NHWC, eight consecutive channels = one 16-byte chunk
// (sepconv.hip's lane layout: lanes are (chunk, pixel lane) with the chunk fastest), arithmetic fp32.  Rate-major operands: w [4][9][C],
// bias [4][C], z / D [4][N, H, W, C], mean / rstd / gamma [4][C], sums [4][2C].
//
//   jp_fwd:  a workgroup owns an 8 x 16 pixel tile of one sample and CG channel chunks and walks `tstep` tiles down the image.  Per tile it stages
//            the tile plus a halo of 8 (24 x 32 pixels) of x in LDS ONCE, as fp32; the window serves all four rates.  z_r = dw_r(x) + b_r is
//            written per rate; training statistics are fixed-order per-workgroup partials [part][4][2C] (sum z, sum z^2 of the STORED z) that a
//            second launch sums in part order into four iseg_bn_stats messages [sum | sum^2 | count].
//   jp_bwd:  D_r = dV_r W'_r^T = gamma rstd du; dz_r = D_r + alpha_r + beta'_r z_r (training statistics: beta' = -gamma rstd^2 dgamma / n,
//            alpha = -gamma rstd dbeta / n - beta' mean; moving statistics: dz_r = D_r).  Rate by rate the workgroup stages dz_r of each of its
//            tiles with its halo of r in LDS and gathers, per INPUT pixel, dx += dw_r^T(dz_r) into registers that live across the four rates
//            (8 floats per tile of the walk), dw_r[tap] += x dz_r and db_r += dz_r (the centre tap: input and output pixels coincide at stride 1).
//            dx is stored once after the last rate; dz never reaches global memory and no per-rate dx exists.  The weight and bias gradients
//            are per-workgroup partials [part][4][10][C] (nine taps, then the bias) summed in part order into dw / db (+=).
//            Under training statistics the bias gradient is identically zero -- sum dz_r = sum D_r - gamma rstd dbeta + beta' (sum z_r - n mean),
//            and sum D_r = gamma rstd dbeta, sum z_r = n mean over the batch the statistics come from (over all replicas under SyncBN, where the
//            gradient all-reduce forms that sum) -- so the kernel adds nothing to db then, instead of the rounding of D_r and W'_r (bf16: a few
//            1e-3 of dbeta, measured against 1e-3 .. 2e-3 on the composed route, whose own value is rounding noise as well).
//
// The loop order of jp_bwd (rate outside, tile walk inside) is what keeps one launch inside the register file: the per-rate accumulators
// (10 x 8 floats) are reduced and reused after each rate, and the data gradient carries 8 floats per walked tile instead of the weight
// gradient carrying 4 x 10 x 8.  The price is that x is read once per rate (from L2 after the first).
//
// The tiling depends on the shape only and every sum runs in an order fixed by it: no float atomics, bit-reproducible.
#include "common.h"

namespace {

constexpr int JP_THREADS = 256;
constexpr int JP_RATES = 4;                        // dilation 1 << r
constexpr int JP_TH = 8, JP_TW = 16;               // pixel tile
constexpr int JP_HALO = 8;                         // the largest rate
constexpr int JP_RH = JP_TH + 2 * JP_HALO;         // 24
constexpr int JP_RW = JP_TW + 2 * JP_HALO;         // 32
constexpr int JP_CG_MAX = 2;                       // chunks per workgroup: 24 x 32 x 2 x 32 B = 48 KiB of LDS
constexpr int JP_WIDTH_MAX = JP_CG_MAX * 8;        // channels per workgroup
constexpr int JP_TSTEP_MAX = 8;                    // tiles a workgroup walks (jp_bwd keeps 8 floats of dx per walked tile in registers)
constexpr int JP_PART_TARGET = 64;                 // walk further down while there are more partial rows than this
constexpr int JP_BWD_ROWS = 10;                    // nine taps + the bias
constexpr int64_t JP_MAX_PARTS = 1 << 20;

struct JpGeom {
    int N, H, W, C;
    int CG, nchunks, groups, tiles_h, tiles_w, tstep, hsteps;
};

JpGeom jp_geom(int N, int H, int W, int C);
int64_t jp_parts(const JpGeom& g);

bool jp_shape_ok(int N, int H, int W, int C) {
    if (!(N > 0 && N <= 65535 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C / 8 <= 65535 * JP_CG_MAX)) return false;
    return jp_parts(jp_geom(N, H, W, C)) <= JP_MAX_PARTS;      // (also bounds gridDim.x = parts / N)
}

JpGeom jp_geom(int N, int H, int W, int C) {
    JpGeom g;
    g.N = N; g.H = H; g.W = W; g.C = C;
    g.nchunks = C / 8;
    g.CG = g.nchunks >= JP_CG_MAX ? JP_CG_MAX : 1;
    g.groups = (g.nchunks + g.CG - 1) / g.CG;
    g.tiles_h = (H + JP_TH - 1) / JP_TH;
    g.tiles_w = (W + JP_TW - 1) / JP_TW;
    const int64_t cols = (int64_t)N * g.tiles_w;
    g.tstep = 1;
    while (g.tstep < g.tiles_h && g.tstep < JP_TSTEP_MAX && cols * ((g.tiles_h + g.tstep - 1) / g.tstep) > JP_PART_TARGET) g.tstep *= 2;
    g.hsteps = (g.tiles_h + g.tstep - 1) / g.tstep;
    return g;
}

int64_t jp_parts(const JpGeom& g) { return (int64_t)g.N * g.hsteps * g.tiles_w; }
size_t jp_lds_bytes(const JpGeom& g) { return (size_t)JP_RH * JP_RW * g.CG * 8 * sizeof(float); }
bool jp_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define JP_UNSUPPORTED(what, N, H, W, C)                                                                                                    \
    do {                                                                                                                                    \
        iseg_set_error("%s: unsupported shape N=%d H=%d W=%d C=%d (C %% 8 == 0, N <= 65535, 16-byte aligned tensors)", what, N, H, W, C);  \
        return ISEG_ERR_UNSUPPORTED;                                                                                                        \
    } while (0)

// `rows` x `width` per-channel values ([rate][tap][channel] or [rate][channel]) of the workgroup's channels into LDS (zeros past C)
__device__ __forceinline__ void jp_stage_rows(const float* __restrict__ src, float* dst, int rows, int C, int ch0, int width) {
    for (int i = threadIdx.x; i < rows * width; i += JP_THREADS) {
        const int k = i / width, cc = i % width;
        dst[i] = ch0 + cc < C ? src[(int64_t)k * C + ch0 + cc] : 0.f;
    }
}

// Sum ROWS per-lane 8-vectors over the pixel lanes of each chunk into dst[k * C + channel] (k < ROWS).  Inside a wave the lanes of one chunk are
// CG apart: a butterfly over the lane offsets 32 .. CG; the four waves' sums are then added in wave order through LDS.  Every step is fixed by the
// lane layout.  All threads of the workgroup must call this.
template <int ROWS>
__device__ __forceinline__ void jp_block_sums(float (*red)[JP_BWD_ROWS][JP_WIDTH_MAX], const float (*v)[8], int CG, int ch0, int C,
                                              float* __restrict__ dst) {
    const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
    __syncthreads();      // the previous use of red is over
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float s = v[k][e];
            for (int o = 32; o >= CG; o >>= 1) s += __shfl_xor(s, o, 64);
            if (wl < CG) red[wave][k][wl * 8 + e] = s;
        }
    }
    __syncthreads();
    const int width = CG * 8;
    if ((int)threadIdx.x < ROWS * width) {
        const int k = threadIdx.x / width, cc = threadIdx.x % width;
        const float sum = ((red[0][k][cc] + red[1][k][cc]) + red[2][k][cc]) + red[3][k][cc];
        if (ch0 + cc < C) dst[(int64_t)k * C + ch0 + cc] = sum;
    }
}

// ---- forward: z_r = dw3x3_r(x) + bias_r for the four rates from one staged window, optional per-part statistics partials ----------------------
template <class T, bool STATS>
__global__ __launch_bounds__(JP_THREADS) void jp_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            T* __restrict__ z, float* __restrict__ partials, float* __restrict__ packed, JpGeom g) {
    extern __shared__ float4 jp_dyn[];
    float* win = reinterpret_cast<float*>(jp_dyn);
    __shared__ float wsh[JP_RATES * 9 * JP_WIDTH_MAX];
    __shared__ float bsh[JP_RATES * JP_WIDTH_MAX];
    __shared__ float red[JP_THREADS / 64][JP_BWD_ROWS][JP_WIDTH_MAX];
    const int CG = g.CG, C = g.C, width = CG * 8;
    const int c = threadIdx.x % CG, lane = threadIdx.x / CG, lanes = JP_THREADS / CG;
    const int tw_i = blockIdx.x % g.tiles_w, hs = blockIdx.x / g.tiles_w, n = blockIdx.y;
    const int chunk = blockIdx.z * CG + c, ch0 = blockIdx.z * CG * 8;
    const bool chunk_ok = chunk < g.nchunks;
    jp_stage_rows(w, wsh, JP_RATES * 9, C, ch0, width);
    jp_stage_rows(bias, bsh, JP_RATES, C, ch0, width);
    float st[JP_RATES * 2][8];
#pragma unroll
    for (int k = 0; k < JP_RATES * 2; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) st[k][e] = 0.f;
    const int64_t plane = (int64_t)g.H * g.W;
    const T* xn = x + (int64_t)n * plane * C;
    const int w0 = tw_i * JP_TW;
    for (int ts = 0; ts < g.tstep; ++ts) {
        const int th_i = hs * g.tstep + ts;
        if (th_i >= g.tiles_h) break;
        const int h0 = th_i * JP_TH;
        __syncthreads();      // the previous tile's window (and the taps, the first time) are no longer read / are written
        for (int i = threadIdx.x; i < JP_RH * JP_RW * CG; i += JP_THREADS) {
            const int cc = i % CG, rr = i / CG;
            const int h = h0 - JP_HALO + rr / JP_RW, ww = w0 - JP_HALO + rr % JP_RW;
            const int ck = blockIdx.z * CG + cc;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (ck < g.nchunks && h >= 0 && h < g.H && ww >= 0 && ww < g.W) load8<T>(xn + ((int64_t)h * g.W + ww) * C + ck * 8, v);
            float* dst = win + (size_t)i * 8;
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        if (!chunk_ok) continue;
        for (int px = lane; px < JP_TH * JP_TW; px += lanes) {
            const int ho = h0 + px / JP_TW, wo = w0 + px % JP_TW;
            if (ho >= g.H || wo >= g.W) continue;
            const int rb = px / JP_TW + JP_HALO, cb = px % JP_TW + JP_HALO;      // the pixel in window coordinates
#pragma unroll
            for (int r = 0; r < JP_RATES; ++r) {
                const int d = 1 << r;
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = bsh[r * width + c * 8 + e];
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int row = rb + (k / 3 - 1) * d, col = cb + (k % 3 - 1) * d;      // within [0, 24) x [0, 32): |offset| <= 8 = the halo
                    const float* src = win + ((size_t)(row * JP_RW + col) * CG + c) * 8;
                    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
                    const float* wk = &wsh[(r * 9 + k) * width + c * 8];
                    acc[0] = fmaf(a.x, wk[0], acc[0]); acc[1] = fmaf(a.y, wk[1], acc[1]);
                    acc[2] = fmaf(a.z, wk[2], acc[2]); acc[3] = fmaf(a.w, wk[3], acc[3]);
                    acc[4] = fmaf(b.x, wk[4], acc[4]); acc[5] = fmaf(b.y, wk[5], acc[5]);
                    acc[6] = fmaf(b.z, wk[6], acc[6]); acc[7] = fmaf(b.w, wk[7], acc[7]);
                }
                float zr[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) zr[e] = to_f32(from_f32<T>(acc[e]));      // statistics of the stored z (what the GEMM reads)
                store8<T>(z + ((((int64_t)r * g.N + n) * g.H + ho) * g.W + wo) * C + chunk * 8, zr);
                if (STATS) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        st[2 * r][e] += zr[e];
                        st[2 * r + 1][e] = fmaf(zr[e], zr[e], st[2 * r + 1][e]);
                    }
                }
            }
        }
    }
    if (!STATS) return;
    const int64_t part = ((int64_t)n * g.hsteps + hs) * g.tiles_w + tw_i;
    jp_block_sums<JP_RATES * 2>(red, st, CG, ch0, C, partials + part * (JP_RATES * 2) * C);
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < JP_RATES)
        packed[(int64_t)threadIdx.x * (2 * C + 1) + 2 * C] = (float)((int64_t)g.N * plane);
}

// ---- backward: dx = sum_r dw3x3_r^T(dz_r) in registers across the rates; per-part partials of dw_r and db_r; dz_r staged in LDS --------------
template <class T>
__global__ __launch_bounds__(JP_THREADS) void jp_bwd_kernel(const T* __restrict__ D, const T* __restrict__ z, const T* __restrict__ x,
                                                            const float* __restrict__ w, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ sums, float inv_n, int train,
                                                            T* __restrict__ dx, float* __restrict__ partials, JpGeom g) {
    extern __shared__ float4 jp_dyn[];
    float* win = reinterpret_cast<float*>(jp_dyn);
    __shared__ float wsh[JP_RATES * 9 * JP_WIDTH_MAX];
    __shared__ float coef[JP_RATES][2][JP_WIDTH_MAX];      // alpha, beta' of the workgroup's channels, per rate
    __shared__ float red[JP_THREADS / 64][JP_BWD_ROWS][JP_WIDTH_MAX];
    const int CG = g.CG, C = g.C, width = CG * 8;
    const int c = threadIdx.x % CG, px = threadIdx.x / CG;      // one pixel of the 8 x 16 tile per lane (CG = 1: the upper half of the lanes idles)
    const int tw_i = blockIdx.x % g.tiles_w, hs = blockIdx.x / g.tiles_w, n = blockIdx.y;
    const int chunk = blockIdx.z * CG + c, ch0 = blockIdx.z * CG * 8;
    const int w0 = tw_i * JP_TW;
    const int py = px / JP_TW, pxc = px % JP_TW;
    const bool lane_ok = chunk < g.nchunks && px < JP_TH * JP_TW && w0 + pxc < g.W;
    jp_stage_rows(w, wsh, JP_RATES * 9, C, ch0, width);
    if ((int)threadIdx.x < JP_RATES * width) {
        const int r = threadIdx.x / width, cc = threadIdx.x % width, ch = ch0 + cc;
        float al = 0.f, bp = 0.f;
        if (train && ch < C) {
            const int64_t k = (int64_t)r * C + ch;
            const float gr = gamma[k] * rstd[k];
            bp = -gr * rstd[k] * sums[(int64_t)r * 2 * C + C + ch] * inv_n;
            al = -gr * sums[(int64_t)r * 2 * C + ch] * inv_n - bp * mean[k];
        }
        coef[r][0][cc] = al;
        coef[r][1][cc] = bp;
    }
    float acc[JP_TSTEP_MAX][8];
#pragma unroll
    for (int ts = 0; ts < JP_TSTEP_MAX; ++ts)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[ts][e] = 0.f;
    const int64_t plane = (int64_t)g.H * g.W;
    const int64_t part = ((int64_t)n * g.hsteps + hs) * g.tiles_w + tw_i;
#pragma unroll
    for (int r = 0; r < JP_RATES; ++r) {
        const int d = 1 << r;
        const int RHd = JP_TH + 2 * d, RWd = JP_TW + 2 * d;      // the tile plus its halo of d: at most 24 x 32, the staged region's size
        const int64_t rbase = ((int64_t)r * g.N + n) * plane;
        float dwacc[JP_BWD_ROWS][8];
#pragma unroll
        for (int k = 0; k < JP_BWD_ROWS; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) dwacc[k][e] = 0.f;
#pragma unroll
        for (int ts = 0; ts < JP_TSTEP_MAX; ++ts) {
            const int th_i = hs * g.tstep + ts;
            if (ts < g.tstep && th_i < g.tiles_h) {      // uniform over the workgroup
                const int h0 = th_i * JP_TH;
                __syncthreads();      // the previous window (and the taps and coefficients, the first time) are no longer read / are written
                for (int i = threadIdx.x; i < RHd * RWd * CG; i += JP_THREADS) {
                    const int cc = i % CG, rr = i / CG;
                    const int ho = h0 - d + rr / RWd, wo = w0 - d + rr % RWd;
                    const int ck = blockIdx.z * CG + cc;
                    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (ck < g.nchunks && ho >= 0 && ho < g.H && wo >= 0 && wo < g.W) {
                        const int64_t off = (rbase + (int64_t)ho * g.W + wo) * C + ck * 8;
                        float dv[8], zv[8];
                        load8<T>(D + off, dv);
                        load8<T>(z + off, zv);
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = fmaf(coef[r][1][cc * 8 + e], zv[e], dv[e] + coef[r][0][cc * 8 + e]);
                    }
                    float* dst = win + (size_t)i * 8;
                    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                }
                __syncthreads();
                const int h = h0 + py;
                if (lane_ok && h < g.H) {
                    float xv[8];
                    load8<T>(x + (((int64_t)n * g.H + h) * g.W + w0 + pxc) * C + chunk * 8, xv);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            // dz at (h - (i - 1) d, w - (j - 1) d); the window starts at (h0 - d, w0 - d): rows [0, 8 + 2d), columns [0, 16 + 2d)
                            const int row = py + (2 - i) * d, col = pxc + (2 - j) * d;
                            const float* src = win + ((size_t)(row * RWd + col) * CG + c) * 8;
                            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
                            const float dz[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                            const float* wk = &wsh[(r * 9 + i * 3 + j) * width + c * 8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                acc[ts][e] = fmaf(wk[e], dz[e], acc[ts][e]);
                                dwacc[i * 3 + j][e] = fmaf(xv[e], dz[e], dwacc[i * 3 + j][e]);
                            }
                            if (i == 1 && j == 1 && !train) {      // (training statistics: sum dz_r is identically zero, see the header comment)
#pragma unroll
                                for (int e = 0; e < 8; ++e) dwacc[9][e] += dz[e];
                            }
                        }
                    }
                }
            }
        }
        jp_block_sums<JP_BWD_ROWS>(red, dwacc, CG, ch0, C, partials + (part * JP_RATES + r) * JP_BWD_ROWS * C);
    }
#pragma unroll
    for (int ts = 0; ts < JP_TSTEP_MAX; ++ts) {
        const int th_i = hs * g.tstep + ts;
        const int h = th_i * JP_TH + py;
        if (ts < g.tstep && th_i < g.tiles_h && lane_ok && h < g.H)
            store8<T>(dx + (((int64_t)n * g.H + h) * g.W + w0 + pxc) * C + chunk * 8, acc[ts]);
    }
}

}  // namespace

extern "C" int iseg_jpu_supported(int N, int H, int W, int C, int dtype) {
    return jp_shape_ok(N, H, W, C) && (dtype == ISEG_F32 || dtype == ISEG_BF16) ? 1 : 0;
}

// partial rows of one launch: forward [part][4][2C], backward [part][4][10][C] floats
extern "C" size_t iseg_jpu_partials_bytes(int N, int H, int W, int C, int backward) {
    if (!jp_shape_ok(N, H, W, C)) return 0;
    return (size_t)jp_parts(jp_geom(N, H, W, C)) * JP_RATES * (backward ? JP_BWD_ROWS : 2) * C * sizeof(float);
}

extern "C" int iseg_jpu_dwconv3x4_stats(const void* x, const float* w, const float* bias, void* z, float* packed, int N, int H, int W, int C,
                                        int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && w && bias && z, "iseg_jpu_dwconv3x4_stats: null pointer");
    if (!jp_shape_ok(N, H, W, C) || !jp_aligned(x) || !jp_aligned(w) || !jp_aligned(bias) || !jp_aligned(z))
        JP_UNSUPPORTED("iseg_jpu_dwconv3x4_stats", N, H, W, C);
    if (packed) ISEG_NEED_WORKSPACE("iseg_jpu_dwconv3x4_stats", ws, ws_bytes, iseg_jpu_partials_bytes(N, H, W, C, 0));
    const JpGeom g = jp_geom(N, H, W, C);
    const dim3 grid(g.tiles_w * g.hsteps, N, g.groups);
    const size_t lds = jp_lds_bytes(g);
    float* part = (float*)ws;
    const int rc = by_dtype(dtype, "iseg_jpu_dwconv3x4_stats", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL((packed ? jp_fwd_kernel<T, true> : jp_fwd_kernel<T, false>), grid, dim3(JP_THREADS), lds, stream, (const T*)x, w, bias,
                           (T*)z, packed ? part : nullptr, packed, g);
    });
    if (rc != ISEG_OK) return rc;
    // [part][4][2C] -> packed [4][2C+1]: one batch entry per rate, the count slot (written by the kernel) skipped by the output stride
    if (packed)
        launch_reduce_rows({.partials = part, .P = (int)jp_parts(g), .pstride = JP_RATES * 2 * (int64_t)C, .n = 2 * (int64_t)C, .out0 = packed,
                            .n0 = 2 * (int64_t)C, .batch = JP_RATES, .bstride_in = 2 * (int64_t)C, .bstride_out = 2 * (int64_t)C + 1}, stream);
    return iseg_check_launch("iseg_jpu_dwconv3x4_stats");
}

extern "C" int iseg_jpu_bnfold_dwconv3x4_bwd(const void* D, const void* z, const void* x, const float* w, const float* mean, const float* rstd,
                                             const float* gamma, const float* sums, float inv_n, int train, void* dx, float* dw, float* db, int N,
                                             int H, int W, int C, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(D && z && x && w && dx && dw && db, "iseg_jpu_bnfold_dwconv3x4_bwd: null pointer");
    ISEG_REQUIRE(!train || (mean && rstd && gamma && sums), "iseg_jpu_bnfold_dwconv3x4_bwd: training statistics need mean, rstd, gamma, sums");
    if (!jp_shape_ok(N, H, W, C) || !jp_aligned(D) || !jp_aligned(z) || !jp_aligned(x) || !jp_aligned(w) || !jp_aligned(dx))
        JP_UNSUPPORTED("iseg_jpu_bnfold_dwconv3x4_bwd", N, H, W, C);
    ISEG_NEED_WORKSPACE("iseg_jpu_bnfold_dwconv3x4_bwd", ws, ws_bytes, iseg_jpu_partials_bytes(N, H, W, C, 1));
    const JpGeom g = jp_geom(N, H, W, C);
    const dim3 grid(g.tiles_w * g.hsteps, N, g.groups);
    const size_t lds = jp_lds_bytes(g);
    float* part = (float*)ws;
    const int rc = by_dtype(dtype, "iseg_jpu_bnfold_dwconv3x4_bwd", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(jp_bwd_kernel<T>, grid, dim3(JP_THREADS), lds, stream, (const T*)D, (const T*)z, (const T*)x, w, mean, rstd, gamma, sums,
                           inv_n, train, (T*)dx, part, g);
    });
    if (rc != ISEG_OK) return rc;
    // [part][4][10][C]: rows 0..8 of every rate -> dw [4][9][C], row 9 -> db [4][C]; one batch entry per rate
    const int64_t prow = JP_RATES * JP_BWD_ROWS * (int64_t)C, rrow = JP_BWD_ROWS * (int64_t)C;
    launch_reduce_rows({.partials = part, .P = (int)jp_parts(g), .pstride = prow, .n = 9 * (int64_t)C, .out0 = dw, .n0 = 9 * (int64_t)C, .accumulate = 1,
                        .batch = JP_RATES, .bstride_in = rrow, .bstride_out = 9 * (int64_t)C}, stream);
    launch_reduce_rows({.partials = part + 9 * (int64_t)C, .P = (int)jp_parts(g), .pstride = prow, .n = C, .out0 = db, .n0 = C, .accumulate = 1,
                        .batch = JP_RATES, .bstride_in = rrow, .bstride_out = C}, stream);
    return iseg_check_launch("iseg_jpu_bnfold_dwconv3x4_bwd");
}
