// Normalisation kernels (HBM-bound): LayerNorm over the channel axis and (Sync)BatchNorm over N,H,W.
//
// LayerNorm follows keras.layers.LayerNormalization(axis=-1, epsilon) as used by backbones/convnext.py:27,71,
// backbones/swin.py (norm1/norm2/PatchMerging.norm) and backbones/vit.py: biased variance, fp32 statistics,
// (x-mean)*rsqrt(var+eps)*gamma+beta.  BatchNorm follows the synchronized moments path of
// layers/keras3/bn.py:10-73 / layers/syncbn.py:70-119: per-replica sum, sum of squares and count are reduced
// (here: packed as one [2C+1] fp32 message for a single RCCL all-reduce), mean = S1/n, var = S2/n - mean^2.
#include <stdlib.h>

#include "common.h"
#include "iseg_hip.h"

namespace {

constexpr int LN_MAX_CHUNKS = 8;  // 8-element chunks per lane kept in registers

// Optional tail of a post-norm residual branch (backbones/intern_image/intern_image.py:226-236: x = residual + drop_path(gamma_ls * norm(f(x)))):
// y = residual + rowscale[row / rows_per_group] * colscale[c] * LayerNorm(x).  All-NULL = plain LayerNorm.
struct LnPost {
    const float* colscale;      // layer scale, [C] (NULL: 1)
    const float* rowscale;      // drop-path factor per group of rows_per_group rows (NULL: 1)
    int64_t rows_per_group;
    const void* residual;       // [rows, C] in the activation dtype (NULL: none)
};

// lanes per row: smallest power of two >= number of 8-element chunks, capped at 64.  `thirds` (the forward kernel at the narrow ConvNeXt / Swin
// widths 96 and 192: 12 / 24 chunks): 4 / 8 lanes with three chunks each instead of 16 / 32 lanes with a quarter of them idle -- measured
// (tools/kbench_ln.py, 16 images) forward 22.0 -> 17.6 us at 128 x 128 x 96 and 13.4 -> 11.0 at 64 x 64 x 192, equal at 384 / 768; the backward kernel
// LOSES with it at every width (39 -> 59, 26 -> 32, 19.5 -> 22.9, 16.5 -> 19.3 us: 144 more registers of rows in flight) and keeps the old split.
static inline int ln_lanes_per_row(int C, bool thirds = false) {
    const int chunks = (C + 7) / 8;
    if (thirds && chunks % 3 == 0 && chunks <= 24) {
        const int t = chunks / 3;
        if (t >= 1 && (t & (t - 1)) == 0) return t;
    }
    int l = 1;
    while (l < chunks && l < 64) l <<= 1;
    return l;
}


// ------------------------------------------------------------------------------------------------
// LayerNorm forward: `LPR` lanes cooperate on one row, 64/LPR rows per wave, values stay in registers
// ------------------------------------------------------------------------------------------------
template <class T, int CPL, bool POST = false>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ y,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                            int64_t rows, int C, float eps, int lpr, const int32_t* __restrict__ src_index,
                                                            LnPost post) {
    // src_index (optional): output row r is LayerNorm(x[src_index[r]]), or a row of ZEROS where src_index[r] < 0 -- Swin's norm1 followed by
    // zero-pad + cyclic roll + window partition (backbones/swin.py:246-262) in one pass; statistics are then kept per OUTPUT row
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int rpw = 64 / lpr;  // rows per wave
    const int sub = lane / lpr, li = lane % lpr;
    const int nchunks = C / 8;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wid;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    // a lane always owns the same channel chunks: gamma / beta live in registers for the whole strip (loading them per row was a second
    // dependent round trip per row), and the row loads are issued unconditionally from clamped addresses (a branch per load makes hipcc
    // wait for each one)
    float g[CPL][8], bt[CPL][8];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = li + i * lpr;
        const int cc = c < nchunks ? c : nchunks - 1;
        load8<float>(gamma + cc * 8, g[i]);
        load8<float>(beta + cc * 8, bt[i]);
        if (POST && post.colscale) {      // the layer scale folds into the affine pair: cs * (xhat g + b) = xhat (cs g) + cs b
            float cs[8];
            load8<float>(post.colscale + cc * 8, cs);
#pragma unroll
            for (int u = 0; u < 8; ++u) g[i][u] *= cs[u], bt[i][u] *= cs[u];
        }
    }
    const T* const res = POST ? static_cast<const T*>(post.residual) : nullptr;      // (POST = false: the plain kernel carries none of the tail)
    for (int64_t rbase = wave_global * rpw; rbase < rows; rbase += nwaves * rpw) {
        const int64_t row = rbase + sub;
        const bool valid = row < rows;
        int64_t rc = valid ? row : rows - 1;
        bool pad_row = false;
        if (src_index) {
            const int32_t src = src_index[rc];
            pad_row = src < 0;
            rc = pad_row ? 0 : src;
        }
        float v[CPL][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = li + i * lpr;
            const bool ok = valid && c < nchunks;
            load8<T>(x + rc * C + (c < nchunks ? c : nchunks - 1) * 8, v[i]);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[i][u] = ok ? v[i][u] : 0.f;
                s += v[i][u];
            }
        }
        s = group_sum(s, lpr);
        const float mean = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = li + i * lpr;
            if (valid && c < nchunks) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float d = v[i][u] - mean;
                    q += d * d;
                }
            }
        }
        q = group_sum(q, lpr);
        const float rstd = rsqrtf(q / (float)C + eps);
        const float rsf = POST && post.rowscale && valid ? post.rowscale[row / post.rows_per_group] : 1.f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = li + i * lpr;
            if (valid && c < nchunks) {
                float o[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) o[u] = pad_row ? 0.f : (v[i][u] - mean) * rstd * g[i][u] + bt[i][u];
                if (POST && post.rowscale) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) o[u] *= rsf;
                }
                if (res) {
                    float a[8];
                    load8<T>(res + row * C + c * 8, a);
#pragma unroll
                    for (int u = 0; u < 8; ++u) o[u] += a[u];
                }
                store8<T>(y + row * C + c * 8, o);
            }
        }
        if (valid && li == 0) {
            if (mean_out) mean_out[row] = pad_row ? 0.f : mean;
            if (rstd_out) rstd_out[row] = pad_row ? 0.f : rstd;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm backward.
//   g = dy*gamma ; dx = rstd * (g - mean_C(g) - xhat*mean_C(g*xhat))
//   dgamma = sum_rows dy*xhat ; dbeta = sum_rows dy  -> per-block partials [grid][2][C], reduced by colsum2
// Each lane always owns the same channel chunks, so the parameter-gradient partials live in registers for
// the whole row strip and are combined once per block through LDS.
// ------------------------------------------------------------------------------------------------
template <class T, int CPL, int U, bool POST = false>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, T* __restrict__ dx,
                                                            const T* __restrict__ dx_add, float* __restrict__ partials,
                                                            int64_t rows, int C, int lpr, const int32_t* __restrict__ dy_index, LnPost post) {
    // post (a post-norm residual branch, see LnPost): the arriving gradient is taken as rowscale * dy and the affine scale as colscale * gamma;
    // the column sums written to `partials` are then A = sum rowscale dy xhat and B = sum rowscale dy, from which the host-side finish derives
    // dgamma = colscale A, dbeta = colscale B and dcolscale = gamma A + beta B
    // dy_index (optional): the gradient row and the saved statistics of source row r sit at row dy_index[r] (< 0: no gradient arrives) -- the
    // backward of layernorm_fwd_kernel's src_index form with the inverse table
    extern __shared__ __attribute__((aligned(16))) float lds_part[];  // [2][C]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int rpw = 64 / lpr;
    const int sub = lane / lpr, li = lane % lpr;
    const int nchunks = C / 8;
    for (int i = threadIdx.x; i < 2 * C; i += 256) lds_part[i] = 0.f;
    __syncthreads();

    float dg[CPL][8], db[CPL][8], gam[CPL][8];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int c = li + i * lpr;
#pragma unroll
        for (int u = 0; u < 8; ++u) dg[i][u] = db[i][u] = gam[i][u] = 0.f;
        if (c < nchunks) {
            load8<float>(gamma + c * 8, gam[i]);
            if (POST && post.colscale) {
                float cs[8];
                load8<float>(post.colscale + c * 8, cs);
#pragma unroll
                for (int u = 0; u < 8; ++u) gam[i][u] *= cs[u];
            }
        }
    }

    // U rows per lane group are in flight together: with wide rows (one row per wavefront and iteration) the loop is otherwise one dependent
    // L2 / HBM round trip per row (measured 16384 x 384: 29 us for 38 MB)
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wid;
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    for (int64_t rbase = wave_global * rpw * U; rbase < rows; rbase += nwaves * rpw * U) {
        float d[U][CPL][8], xv[U][CPL][8], mu[U], rs[U];
        bool valid[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t row = rbase + q * rpw + sub;
            valid[q] = row < rows;
            // every load is issued unconditionally from a clamped address and zeroed by a select afterwards: a branch per load makes hipcc
            // wait for each one at the join, which serialises the rows again
            const int64_t rc = valid[q] ? row : rows - 1;
            int64_t rd = rc;
            bool has_dy = true;
            if (dy_index) {
                const int32_t j = dy_index[rc];
                has_dy = j >= 0;
                rd = has_dy ? j : 0;
            }
            mu[q] = mean[rd];
            rs[q] = valid[q] && has_dy ? rstd[rd] : 0.f;
            const float rsf = POST && post.rowscale ? post.rowscale[rd / post.rows_per_group] : 1.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = li + i * lpr;
                const bool ok = valid[q] && has_dy && c < nchunks;
                const int cc = c < nchunks ? c : nchunks - 1;
                load8<T>(dy + rd * C + cc * 8, d[q][i]);
                load8<T>(x + rc * C + cc * 8, xv[q][i]);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    d[q][i][u] = ok ? d[q][i][u] * rsf : 0.f;
                    xv[q][i][u] = ok ? xv[q][i][u] : mu[q];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t row = rbase + q * rpw + sub;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float h = (xv[q][i][u] - mu[q]) * rs[q];      // (padding chunks: d = 0, so they add nothing)
                    const float gv = d[q][i][u] * gam[i][u];
                    xv[q][i][u] = h;
                    s1 += gv;
                    s2 += gv * h;
                    dg[i][u] += d[q][i][u] * h;
                    db[i][u] += d[q][i][u];
                    d[q][i][u] = gv;
                }
            s1 = group_sum(s1, lpr) / (float)C;
            s2 = group_sum(s2, lpr) / (float)C;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = li + i * lpr;
                if (valid[q] && c < nchunks) {
                    float o[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) o[u] = rs[q] * (d[q][i][u] - s1 - xv[q][i][u] * s2);
                    if (dx_add) {
                        float a[8];
                        load8<T>(dx_add + row * C + c * 8, a);
#pragma unroll
                        for (int u = 0; u < 8; ++u) o[u] += a[u];
                    }
                    store8<T>(dx + row * C + c * 8, o);
                }
            }
        }
    }
    // block-level combine in a FIXED order (bit-reproducible; reference default use_deterministic=True, core_env.py:39-48): the row sub-groups
    // of a wavefront meet by lane exchanges, then wavefront 0 stores its sums and wavefronts 1..3 add theirs one after the other
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            // combine the rows-per-wave sub-groups first (same channel, lanes li + k*lpr)
            for (int o = lpr; o < 64; o <<= 1) {
                dg[i][u] += __shfl_xor(dg[i][u], o, 64);
                db[i][u] += __shfl_xor(db[i][u], o, 64);
            }
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wid == w && sub == 0) {
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = li + i * lpr;
                if (c < nchunks) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        lds_part[c * 8 + u] += dg[i][u];
                        lds_part[C + c * 8 + u] += db[i][u];
                    }
                }
            }
        }
        __syncthreads();
    }
    float* out = partials + (int64_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += 256) out[i] = lds_part[i];
}


// ------------------------------------------------------------------------------------------------
// Any width (C not a multiple of 8: rows are not 16-byte aligned).  EVA02-large normalises int(1024 * 8 / 3) = 2730 hidden units
// (backbones/eva/swiglu.py:74-80).  One wavefront per row, lane l owns columns l, l + 64, ...: scalar loads, the same two-pass statistics; the
// backward keeps its column sums in one LDS slab per wavefront (a lane owns its columns there, so no atomics and a fixed order) and writes the
// per-workgroup partials the ordinary reduce consumes.  Plain LayerNorm only (no gather table, no post-norm tail).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <class T>
__global__ __launch_bounds__(256) void layernorm_fwd_any_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                T* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t rows,
                                                                int C, float eps) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wid; row < rows; row += (int64_t)gridDim.x * 4) {
        const T* xr = x + row * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += to_f32(xr[c]);
        const float mean = ln_wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = to_f32(xr[c]) - mean;
            q += d * d;
        }
        const float rstd = rsqrtf(ln_wave_sum(q) / (float)C + eps);
        T* yr = y + row * C;
        for (int c = lane; c < C; c += 64) yr[c] = from_f32<T>((to_f32(xr[c]) - mean) * rstd * gamma[c] + beta[c]);
        if (lane == 0) {
            if (mean_out) mean_out[row] = mean;
            if (rstd_out) rstd_out[row] = rstd;
        }
    }
}

constexpr int LN_ANY_WAVES = 2;      // wavefronts per workgroup of the any-width backward: 2 x 2 x C floats of LDS (C <= 4096: 64 KiB)

template <class T>
__global__ __launch_bounds__(64 * LN_ANY_WAVES) void layernorm_bwd_any_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                               const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                               const float* __restrict__ rstd, T* __restrict__ dx,
                                                                               const T* __restrict__ dx_add, float* __restrict__ partials, int64_t rows,
                                                                               int C) {
    extern __shared__ __attribute__((aligned(16))) float ln_any_slab[];      // [LN_ANY_WAVES][2][C]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float* const sg = ln_any_slab + (size_t)wid * 2 * C;
    float* const sb = sg + C;
    for (int c = lane; c < C; c += 64) sg[c] = sb[c] = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * LN_ANY_WAVES + wid; row < rows; row += (int64_t)gridDim.x * LN_ANY_WAVES) {
        const T* dr = dy + row * C;
        const T* xr = x + row * C;
        const float mu = mean[row], rs = rstd[row];
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = to_f32(dr[c]), h = (to_f32(xr[c]) - mu) * rs, gv = d * gamma[c];
            s1 += gv;
            s2 += gv * h;
            sg[c] += d * h;
            sb[c] += d;
        }
        s1 = ln_wave_sum(s1) / (float)C;
        s2 = ln_wave_sum(s2) / (float)C;
        T* or_ = dx + row * C;
        for (int c = lane; c < C; c += 64) {
            const float d = to_f32(dr[c]), h = (to_f32(xr[c]) - mu) * rs;
            float o = rs * (d * gamma[c] - s1 - h * s2);
            if (dx_add) o += to_f32(dx_add[row * C + c]);
            or_[c] = from_f32<T>(o);
        }
    }
    __syncthreads();
    float* out = partials + (int64_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += 64 * LN_ANY_WAVES) {
        float a = ln_any_slab[i];
#pragma unroll
        for (int w = 1; w < LN_ANY_WAVES; ++w) a += ln_any_slab[(size_t)w * 2 * C + i];
        out[i] = a;
    }
}

static int ln_any_bwd_blocks(int64_t rows) {
    return (int)grid_cap(rows, LN_ANY_WAVES * 4, 512);      // four rows per wavefront at least
}

// parameter gradients of a post-norm residual branch from the two column sums of layernorm_bwd_kernel (see LnPost): sums = [A | B]
__global__ void ln_post_finish_kernel(const float* __restrict__ sums, const float* __restrict__ colscale, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                      float* __restrict__ dcolscale, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float A = sums[c], B = sums[C + c], cs = colscale ? colscale[c] : 1.f;
    dgamma[c] += cs * A;
    dbeta[c] += cs * B;
    if (dcolscale) dcolscale[c] += gamma[c] * A + beta[c] * B;
}

// ------------------------------------------------------------------------------------------------
// BatchNorm
// ------------------------------------------------------------------------------------------------
// per-block partial sums of x and x^2 per channel: block handles a strip of rows; thread owns 8 channels.
template <class T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ x, int64_t ldx, float* __restrict__ partials,
                                                       int64_t rows, int C, float* __restrict__ count_out) {
    extern __shared__ __attribute__((aligned(16))) float lds_s[];  // [rows per iteration][2][C]: one slab row per adder, summed in row order
    const int nchunks = C / 8;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_out = (float)rows;      // packed[2C]: this replica's element count per channel
    // thread t handles chunk (t % tpc) of rows (t / tpc) + k*rows_per_iter
    const int tpc = nchunks < 256 ? nchunks : 256;  // threads across channels
    const int rpi = 256 / tpc;                      // rows per iteration per block
    const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
    const bool active = tr < rpi;
    for (int c = tc; c < nchunks; c += tpc) {
        float s[8] = {}, q[8] = {};
        if (active) {
            // eight rows per trip with their loads issued together (one dependent load per trip waits a memory round trip per row)
            int64_t r = (int64_t)blockIdx.x * rpi + tr;
            const int64_t rstep = (int64_t)gridDim.x * rpi;
            constexpr int UB = 8;
            for (; r + (UB - 1) * rstep < rows; r += UB * rstep) {
                float v[UB][8];
#pragma unroll
                for (int k = 0; k < UB; ++k) load8<T>(x + (r + k * rstep) * ldx + c * 8, v[k]);
#pragma unroll
                for (int k = 0; k < UB; ++k)
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        s[u] += v[k][u];
                        q[u] += v[k][u] * v[k][u];
                    }
            }
            for (; r < rows; r += rstep) {
                float v[8];
                load8<T>(x + r * ldx + c * 8, v);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    s[u] += v[u];
                    q[u] += v[u] * v[u];
                }
            }
            float* slab = lds_s + (size_t)tr * 2 * C;      // (every cell of slab rows 0..rpi-1 is written exactly once)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                slab[c * 8 + u] = s[u];
                slab[C + c * 8 + u] = q[u];
            }
        }
    }
    __syncthreads();
    float* out = partials + (int64_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        float a = lds_s[i];
        for (int t = 1; t < rpi; ++t) a += lds_s[(size_t)t * 2 * C + i];
        out[i] = a;
    }
}

// packed[0:C]=sum, [C:2C]=sumsq, [2C]=count  ->  mean/var(biased), then update moving stats
__global__ void bn_finalize_kernel(const float* __restrict__ packed, int C, float eps, float momentum, float* __restrict__ mean,
                                   float* __restrict__ rstd, float* __restrict__ moving_mean, float* __restrict__ moving_var) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float n = packed[2 * C];
    const float m = packed[c] / n;
    float var = packed[C + c] / n - m * m;
    var = relu_f32(var);      // (cancellation may leave -1e-8; a NaN variance -- a NaN or an infinity in the channel -- stays NaN, as in the reference)
    mean[c] = m;
    rstd[c] = rsqrtf(var + eps);
    if (moving_mean) moving_mean[c] = moving_mean[c] * momentum + m * (1.f - momentum);
    if (moving_var) moving_var[c] = moving_var[c] * momentum + var * (1.f - momentum);
}

// Strip mapping of the element-wise BatchNorm kernels: thread (tc, tr) owns channel chunk(s) tc, tc + tpc, ... (eight channels each) and rows
// blockIdx * rpi + tr, + gridDim * rpi, ... -- the per-channel constants (statistics, gamma, beta; in the packed form two divisions and an rsqrt per
// channel) are derived once per chunk instead of once per 16 bytes of x (bn_apply_packed ran at 2.9 TB/s on those divisions, 5.5 without them).
struct BnStrip {
    int nchunks, tpc, rpi, tc, tr;
    bool active;
    __device__ __forceinline__ BnStrip(int C) {
        nchunks = C / 8;
        tpc = nchunks < 256 ? nchunks : 256;
        rpi = 256 / tpc;
        tc = threadIdx.x % tpc;
        tr = threadIdx.x / tpc;
        active = tr < rpi;
    }
};

// y = act((x-mean)*rstd*gamma+beta), y may be a channel slice of a wider (concat) buffer
template <class T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, T* __restrict__ y, int64_t ldy,
                                                       int64_t rows, int C, int relu) {
    const BnStrip st(C);
    if (!st.active) return;
    const int64_t rstep = (int64_t)gridDim.x * st.rpi;
    for (int cc = st.tc; cc < st.nchunks; cc += st.tpc) {
        const int c = cc * 8;
        float m[8], s[8], g[8], b[8];
        load8<float>(mean + c, m);
        load8<float>(rstd + c, s);
        load8<float>(gamma + c, g);
        load8<float>(beta + c, b);
        int64_t r = (int64_t)blockIdx.x * st.rpi + st.tr;
        constexpr int UB = 4;
        for (; r + (UB - 1) * rstep < rows; r += UB * rstep) {
            float v[UB][8];
#pragma unroll
            for (int k = 0; k < UB; ++k) load8<T>(x + (r + k * rstep) * ldx + c, v[k]);
#pragma unroll
            for (int k = 0; k < UB; ++k) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float o = (v[k][u] - m[u]) * s[u] * g[u] + b[u];
                    if (relu) o = relu_f32(o);
                    v[k][u] = o;
                }
                store8<T>(y + (r + k * rstep) * ldy + c, v[k]);
            }
        }
        for (; r < rows; r += rstep) {
            float v[8];
            load8<T>(x + r * ldx + c, v);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float o = (v[u] - m[u]) * s[u] * g[u] + b[u];
                if (relu) o = relu_f32(o);
                v[u] = o;
            }
            store8<T>(y + r * ldy + c, v);
        }
    }
}

// bn_finalize + bn_apply in one launch: every lane derives mean / rstd of its eight channels from the packed sums with bn_finalize_kernel's
// arithmetic (bit-identical), the lane that owns row 0 of a channel chunk also writes mean, rstd and the moving statistics
template <class T>
__global__ __launch_bounds__(256) void bn_apply_packed_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ packed, float eps,
                                                              float momentum, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ moving_mean,
                                                              float* __restrict__ moving_var, T* __restrict__ y, int64_t ldy, int64_t rows, int C,
                                                              int relu) {
    const BnStrip st(C);
    if (!st.active) return;
    const float n = packed[2 * C];
    const int64_t rstep = (int64_t)gridDim.x * st.rpi;
    for (int cc = st.tc; cc < st.nchunks; cc += st.tpc) {
        const int c = cc * 8;
        float m[8], s[8], g[8], b[8], var[8];
        load8<float>(packed + c, m);
        load8<float>(packed + C + c, var);
        load8<float>(gamma + c, g);
        load8<float>(beta + c, b);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            m[u] = m[u] / n;
            var[u] = relu_f32(var[u] / n - m[u] * m[u]);
            s[u] = rsqrtf(var[u] + eps);
        }
        if (blockIdx.x == 0 && st.tr == 0) {      // the lane that owns row 0 of this chunk
            store8<float>(mean + c, m);
            store8<float>(rstd + c, s);
            if (moving_mean) {
                float mm[8];
                load8<float>(moving_mean + c, mm);
#pragma unroll
                for (int u = 0; u < 8; ++u) mm[u] = mm[u] * momentum + m[u] * (1.f - momentum);
                store8<float>(moving_mean + c, mm);
            }
            if (moving_var) {
                float mv[8];
                load8<float>(moving_var + c, mv);
#pragma unroll
                for (int u = 0; u < 8; ++u) mv[u] = mv[u] * momentum + var[u] * (1.f - momentum);
                store8<float>(moving_var + c, mv);
            }
        }
        int64_t r = (int64_t)blockIdx.x * st.rpi + st.tr;
        constexpr int UB = 4;
        for (; r + (UB - 1) * rstep < rows; r += UB * rstep) {
            float v[UB][8];
#pragma unroll
            for (int k = 0; k < UB; ++k) load8<T>(x + (r + k * rstep) * ldx + c, v[k]);
#pragma unroll
            for (int k = 0; k < UB; ++k) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    float o = (v[k][u] - m[u]) * s[u] * g[u] + b[u];
                    if (relu) o = relu_f32(o);
                    v[k][u] = o;
                }
                store8<T>(y + (r + k * rstep) * ldy + c, v[k]);
            }
        }
        for (; r < rows; r += rstep) {
            float v[8];
            load8<T>(x + r * ldx + c, v);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float o = (v[u] - m[u]) * s[u] * g[u] + b[u];
                if (relu) o = relu_f32(o);
                v[u] = o;
            }
            store8<T>(y + r * ldy + c, v);
        }
    }
}

// backward reductions: partial [2][C] = (sum dz, sum dz*xhat) with dz = dy * relu'(y)
template <class T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x,
                                                            int64_t ldx, const T* __restrict__ y, int64_t ldy,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ partials, int64_t rows, int C, int relu,
                                                            const float* __restrict__ re_gamma, const float* __restrict__ re_beta) {
    // re_gamma / re_beta (with relu): the forward output was not kept -- the ReLU mask is re-derived from x, (x - mean) * rstd * gamma + beta > 0
    // with the forward's own expression (y = NULL)
    extern __shared__ __attribute__((aligned(16))) float lds_s[];      // [rows per iteration][2][C], as in bn_stats_kernel
    const int nchunks = C / 8;
    const int tpc = nchunks < 256 ? nchunks : 256;
    const int rpi = 256 / tpc;
    const int tc = threadIdx.x % tpc, tr = threadIdx.x / tpc;
    const bool active = tr < rpi;
    for (int c = tc; c < nchunks; c += tpc) {
        float s[8] = {}, q[8] = {};
        if (active) {
            float m[8], rs[8], rg[8], rb[8];
            load8<float>(mean + c * 8, m);
            load8<float>(rstd + c * 8, rs);
            const bool recompute = relu && re_gamma;
            if (recompute) {
                load8<float>(re_gamma + c * 8, rg);
                load8<float>(re_beta + c * 8, rb);
            }
            int64_t r = (int64_t)blockIdx.x * rpi + tr;
            const int64_t rstep = (int64_t)gridDim.x * rpi;
            constexpr int UB = 4;      // four rows per trip, all of their loads issued together
            for (; r + (UB - 1) * rstep < rows; r += UB * rstep) {
                float d[UB][8], xv[UB][8], yv[UB][8];
#pragma unroll
                for (int k = 0; k < UB; ++k) {
                    load8<T>(dy + (r + k * rstep) * lddy + c * 8, d[k]);
                    load8<T>(x + (r + k * rstep) * ldx + c * 8, xv[k]);
                    if (relu && !recompute) load8<T>(y + (r + k * rstep) * ldy + c * 8, yv[k]);
                }
                if (recompute) {
#pragma unroll
                    for (int k = 0; k < UB; ++k)
#pragma unroll
                        for (int u = 0; u < 8; ++u) yv[k][u] = (xv[k][u] - m[u]) * rs[u] * rg[u] + rb[u];
                }
#pragma unroll
                for (int k = 0; k < UB; ++k)
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float dv = (relu && !(yv[k][u] > 0.f)) ? 0.f : d[k][u];
                        s[u] += dv;
                        q[u] += dv * (xv[k][u] - m[u]) * rs[u];
                    }
            }
            for (; r < rows; r += rstep) {
                float d[8], xv[8];
                load8<T>(dy + r * lddy + c * 8, d);
                load8<T>(x + r * ldx + c * 8, xv);
                if (relu) {
                    float yv[8];
                    if (recompute) {
#pragma unroll
                        for (int u = 0; u < 8; ++u) yv[u] = (xv[u] - m[u]) * rs[u] * rg[u] + rb[u];
                    } else {
                        load8<T>(y + r * ldy + c * 8, yv);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) d[u] = yv[u] > 0.f ? d[u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    s[u] += d[u];
                    q[u] += d[u] * (xv[u] - m[u]) * rs[u];
                }
            }
            float* slab = lds_s + (size_t)tr * 2 * C;      // (every cell of slab rows 0..rpi-1 is written exactly once)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                slab[c * 8 + u] = s[u];
                slab[C + c * 8 + u] = q[u];
            }
        }
    }
    __syncthreads();
    float* out = partials + (int64_t)blockIdx.x * 2 * C;
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        float a = lds_s[i];
        for (int t = 1; t < rpi; ++t) a += lds_s[(size_t)t * 2 * C + i];
        out[i] = a;
    }
}

// dx = gamma*rstd * (dz - sum_dz/n - xhat*sum_dzxhat/n) ; sums[0:C]=sum dz, [C:2C]=sum dz*xhat (already all-reduced).  Strip mapping (BnStrip).
template <class T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, int64_t lddy, const T* __restrict__ x,
                                                           int64_t ldx, const T* __restrict__ y, int64_t ldy,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ sums,
                                                           float inv_n, T* __restrict__ dx, int64_t lddx, int64_t rows, int C,
                                                           int relu, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           const float* __restrict__ re_beta) {
    // re_beta (with relu): the ReLU mask is re-derived from x as in bn_bwd_reduce_kernel (y = NULL)
    const BnStrip st(C);
    if (!st.active) return;
    const int64_t rstep = (int64_t)gridDim.x * st.rpi;
    const bool recompute = relu && re_beta;
    for (int cc = st.tc; cc < st.nchunks; cc += st.tpc) {
        const int c = cc * 8;
        float m[8], rs[8], g[8], s1[8], s2[8], rb[8];
        if (recompute) load8<float>(re_beta + c, rb);
        load8<float>(mean + c, m);
        load8<float>(rstd + c, rs);
        load8<float>(gamma + c, g);
        load8<float>(sums + c, s1);
        load8<float>(sums + C + c, s2);
        if (blockIdx.x == 0 && st.tr == 0 && (dgamma || dbeta)) {   // the lane that owns row 0 of a chunk also books the parameter gradients (dbeta | dgamma = sums)
            float acc[8];
            if (dbeta) {
                load8<float>(dbeta + c, acc);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] += s1[u];
                store8<float>(dbeta + c, acc);
            }
            if (dgamma) {
                load8<float>(dgamma + c, acc);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] += s2[u];
                store8<float>(dgamma + c, acc);
            }
        }
        int64_t r = (int64_t)blockIdx.x * st.rpi + st.tr;
        constexpr int UB = 2;
        for (; r + (UB - 1) * rstep < rows; r += UB * rstep) {
            float d[UB][8], xv[UB][8], yv[UB][8];
#pragma unroll
            for (int k = 0; k < UB; ++k) {
                load8<T>(dy + (r + k * rstep) * lddy + c, d[k]);
                load8<T>(x + (r + k * rstep) * ldx + c, xv[k]);
                if (relu && !recompute) load8<T>(y + (r + k * rstep) * ldy + c, yv[k]);
            }
#pragma unroll
            for (int k = 0; k < UB; ++k) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (recompute) yv[k][u] = (xv[k][u] - m[u]) * rs[u] * g[u] + rb[u];
                    const float dv = (relu && !(yv[k][u] > 0.f)) ? 0.f : d[k][u];
                    const float xh = (xv[k][u] - m[u]) * rs[u];
                    d[k][u] = g[u] * rs[u] * (dv - s1[u] * inv_n - xh * s2[u] * inv_n);
                }
                store8<T>(dx + (r + k * rstep) * lddx + c, d[k]);
            }
        }
        for (; r < rows; r += rstep) {
            float d[8], xv[8];
            load8<T>(dy + r * lddy + c, d);
            load8<T>(x + r * ldx + c, xv);
            if (relu) {
                float yv[8];
                if (recompute) {
#pragma unroll
                    for (int u = 0; u < 8; ++u) yv[u] = (xv[u] - m[u]) * rs[u] * g[u] + rb[u];
                } else {
                    load8<T>(y + r * ldy + c, yv);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) d[u] = yv[u] > 0.f ? d[u] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float xh = (xv[u] - m[u]) * rs[u];
                d[u] = g[u] * rs[u] * (d[u] - s1[u] * inv_n - xh * s2[u] * inv_n);
            }
            store8<T>(dx + r * lddx + c, d);
        }
    }
}

}  // namespace

static int layernorm_fwd_launch(const void* x, const int32_t* src_index, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                int64_t rows, int C, float eps, int dtype, hipStream_t stream, const LnPost& post = LnPost{});

extern "C" int iseg_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                  int64_t rows, int C, float eps, int dtype, hipStream_t stream) {
    return layernorm_fwd_launch(x, nullptr, gamma, beta, y, mean, rstd, rows, C, eps, dtype, stream);
}

extern "C" int iseg_layernorm_post_fwd(const void* x, const float* gamma, const float* beta, const float* colscale, const float* rowscale,
                                       int64_t rows_per_group, const void* residual, void* y, float* mean, float* rstd, int64_t rows, int C,
                                       float eps, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(!rowscale || rows_per_group > 0, "iseg_layernorm_post_fwd: rowscale needs rows_per_group > 0");
    ISEG_REQUIRE((((uintptr_t)colscale | (uintptr_t)residual) & 15) == 0, "iseg_layernorm_post_fwd: colscale / residual must be 16-byte aligned");
    return layernorm_fwd_launch(x, nullptr, gamma, beta, y, mean, rstd, rows, C, eps, dtype, stream, LnPost{colscale, rowscale, rows_per_group, residual});
}

extern "C" int iseg_layernorm_gather_fwd(const void* x, const int32_t* src_index, const float* gamma, const float* beta, void* y, float* mean,
                                         float* rstd, int64_t rows_out, int C, float eps, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(src_index, "iseg_layernorm_gather_fwd: null index table");
    return layernorm_fwd_launch(x, src_index, gamma, beta, y, mean, rstd, rows_out, C, eps, dtype, stream);
}

static int layernorm_fwd_launch(const void* x, const int32_t* src_index, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                int64_t rows, int C, float eps, int dtype, hipStream_t stream, const LnPost& post) {
    ISEG_REQUIRE(x && gamma && beta && y, "iseg_layernorm_fwd: null pointer");
    ISEG_REQUIRE(rows > 0 && C > 0, "iseg_layernorm_fwd: empty problem (rows %lld, C %d)", (long long)rows, C);
    if (C % 8 != 0) {      // rows without 16-byte alignment: the one-wavefront-per-row kernel (plain LayerNorm only)
        ISEG_REQUIRE(!src_index && !post.colscale && !post.rowscale && !post.residual, "iseg_layernorm_fwd: C=%d is not a multiple of 8: plain LayerNorm only", C);
        const unsigned nb = grid_cap(rows, 4, 256 * 8);
        return by_dtype(dtype, "iseg_layernorm_fwd", [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((layernorm_fwd_any_kernel<T>), dim3(nb), dim3(256), 0, stream, (const T*)x, gamma, beta, (T*)y, mean, rstd,
                               rows, C, eps);
            return iseg_check_launch("iseg_layernorm_fwd");
        });
    }
    // (bf16 storage only: in fp32 storage the other lane split changes the order of the row sums in the last bit, and the fp32 path is held to
    // bit-exact argmax masks against the oracle at 512 x 512 -- test_cfg2_at_the_benchmark_shape flipped one near-tie with it)
    const int lpr = ln_lanes_per_row(C, dtype == ISEG_BF16);
    ISEG_REQUIRE((C / 8 + lpr - 1) / lpr <= LN_MAX_CHUNKS, "iseg_layernorm_fwd: C=%d too wide (max %d)", C, 64 * 8 * LN_MAX_CHUNKS);
    const int rpw = 64 / lpr;
    const unsigned blocks = grid_cap(rows, (int64_t)rpw * 4, 256 * 8);
    const int cpl = (C / 8 + lpr - 1) / lpr;
    const bool posted = post.colscale || post.rowscale || post.residual;
    return by_dtype(dtype, "iseg_layernorm_fwd", [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto chunks) {
            constexpr int CPL = decltype(chunks)::value;
            hipLaunchKernelGGL((posted ? layernorm_fwd_kernel<T, CPL, true> : layernorm_fwd_kernel<T, CPL, false>), dim3(blocks), dim3(256), 0, stream,
                               (const T*)x, gamma, beta, (T*)y, mean, rstd, rows, C, eps, lpr, src_index, post);
        };
        if (cpl <= 1) launch(IntC<1>{});
        else if (cpl <= 2) launch(IntC<2>{});
        else if (cpl <= 3) launch(IntC<3>{});
        else if (cpl <= 4) launch(IntC<4>{});
        else launch(IntC<8>{});
        return iseg_check_launch("iseg_layernorm_fwd");
    });
}

static int ln_bwd_blocks(int64_t rows, int C) {
    const int lpr = ln_lanes_per_row(C);
    const int rpw = 64 / lpr;
    // every workgroup pays a fixed price (LDS combine, 2C partial sums written and read again by the reduce), so a workgroup takes ~24 K elements
    // (48 KB of bf16 per operand), between 256 and 1024 workgroups.  Measured best (us incl. the reduce): 262144 x 96 -> 1024 workgroups (37),
    // 65536 x 192 -> 512 (25), 16384 x 384 -> 256 (20.7; 2048 workgroups: 31), 4096 x 768 -> 256..512 (19).
    int64_t rows_per_block = 24576 / C;
    if (rows_per_block < rpw * 4) rows_per_block = rpw * 4;
    const unsigned blocks = grid_cap(rows, rows_per_block, 1024);
    return (int)(blocks < 256 ? grid_cap(rows, (int64_t)rpw * 4, 256) : blocks);
}

extern "C" size_t iseg_layernorm_bwd_workspace_bytes(int64_t rows, int C) {
    if (C % 8 != 0) return (size_t)ln_any_bwd_blocks(rows) * 2 * C * sizeof(float);
    return (size_t)ln_bwd_blocks(rows, C) * 2 * C * sizeof(float);
}

static int layernorm_bwd_launch(const void* dy, const int32_t* dy_index, const void* x, const float* gamma, const float* mean, const float* rstd,
                                void* dx, const void* dx_add, float* dgamma, float* dbeta, int accumulate_param_grads, int64_t rows, int C,
                                int dtype, void* ws, size_t ws_bytes, hipStream_t stream, const LnPost& post = LnPost{}, const float* beta = nullptr,
                                float* dcolscale = nullptr);

// backward of iseg_layernorm_post_fwd: dx = LN^T (rowscale colscale dy); dgamma, dbeta and dcolscale (NULL: not wanted) are ACCUMULATED.
// Workspace: iseg_layernorm_bwd_workspace_bytes(rows, C) + 2 C floats.
extern "C" int iseg_layernorm_post_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* colscale,
                                       const float* rowscale, int64_t rows_per_group, const float* mean, const float* rstd, void* dx,
                                       float* dgamma, float* dbeta, float* dcolscale, int64_t rows, int C, int dtype, void* ws, size_t ws_bytes,
                                       hipStream_t stream) {
    ISEG_REQUIRE(beta && (!rowscale || rows_per_group > 0) && (!dcolscale || colscale), "iseg_layernorm_post_bwd: bad arguments");
    ISEG_REQUIRE(((uintptr_t)colscale & 15) == 0, "iseg_layernorm_post_bwd: colscale must be 16-byte aligned");
    // the documented size whether or not this call has a scale (without one the two finish rows are not used): one rule for the caller
    const size_t promised = iseg_layernorm_bwd_workspace_bytes(rows, C) + (size_t)2 * C * sizeof(float);
    if (rows > 0 && C > 0) ISEG_NEED_WORKSPACE("iseg_layernorm_post_bwd", ws, ws_bytes, promised);
    return layernorm_bwd_launch(dy, nullptr, x, gamma, mean, rstd, dx, nullptr, dgamma, dbeta, 1, rows, C, dtype, ws, ws_bytes, stream,
                                LnPost{colscale, rowscale, rows_per_group, nullptr}, beta, dcolscale);
}

extern "C" int iseg_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                  void* dx, const void* dx_add, float* dgamma, float* dbeta, int accumulate_param_grads,
                                  int64_t rows, int C, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    return layernorm_bwd_launch(dy, nullptr, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, accumulate_param_grads, rows, C, dtype, ws, ws_bytes,
                                stream);
}

extern "C" int iseg_layernorm_gather_bwd(const void* dy, const int32_t* dy_index, const void* x, const float* gamma, const float* mean,
                                         const float* rstd, void* dx, const void* dx_add, float* dgamma, float* dbeta,
                                         int accumulate_param_grads, int64_t rows, int C, int dtype, void* ws, size_t ws_bytes,
                                         hipStream_t stream) {
    ISEG_REQUIRE(dy_index, "iseg_layernorm_gather_bwd: null index table");
    return layernorm_bwd_launch(dy, dy_index, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, accumulate_param_grads, rows, C, dtype, ws, ws_bytes,
                                stream);
}

static int layernorm_bwd_launch(const void* dy, const int32_t* dy_index, const void* x, const float* gamma, const float* mean, const float* rstd,
                                void* dx, const void* dx_add, float* dgamma, float* dbeta, int accumulate_param_grads, int64_t rows, int C,
                                int dtype, void* ws, size_t ws_bytes, hipStream_t stream, const LnPost& post, const float* beta, float* dcolscale) {
    ISEG_REQUIRE(dy && x && gamma && mean && rstd && dx && dgamma && dbeta, "iseg_layernorm_bwd: null pointer");
    ISEG_REQUIRE(rows > 0 && C > 0, "iseg_layernorm_bwd: empty problem (rows %lld, C %d)", (long long)rows, C);
    ISEG_REQUIRE(dtype == ISEG_BF16 || dtype == ISEG_F32, "iseg_layernorm_bwd: dtype %d", dtype);      // (before the first launch)
    if (C % 8 != 0) {      // the any-width form (see layernorm_bwd_any_kernel)
        ISEG_REQUIRE(!dy_index && !post.colscale && !post.rowscale && C <= 4096, "iseg_layernorm_bwd: C=%d is not a multiple of 8: plain LayerNorm, C <= 4096", C);
        const int nb = ln_any_bwd_blocks(rows);
        const size_t need_any = (size_t)nb * 2 * C * sizeof(float);
        ISEG_NEED_WORKSPACE("iseg_layernorm_bwd", ws, ws_bytes, need_any);
        float* parts = (float*)ws;
        const size_t lds_any = (size_t)LN_ANY_WAVES * 2 * C * sizeof(float);
        const int rc = by_dtype(dtype, "iseg_layernorm_bwd", [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((layernorm_bwd_any_kernel<T>), dim3(nb), dim3(64 * LN_ANY_WAVES), lds_any, stream, (const T*)dy, (const T*)x, gamma,
                               mean, rstd, (T*)dx, (const T*)dx_add, parts, rows, C);
        });
        if (rc != ISEG_OK) return rc;
        launch_reduce_rows({.partials = parts, .P = nb, .pstride = 2 * C, .n = 2 * C, .out0 = dgamma, .out1 = dbeta, .n0 = C,
                            .accumulate = accumulate_param_grads}, stream);
        return iseg_check_launch("iseg_layernorm_bwd");
    }
    const int lpr = ln_lanes_per_row(C);
    ISEG_REQUIRE((C / 8 + lpr - 1) / lpr <= LN_MAX_CHUNKS, "iseg_layernorm_bwd: C=%d too wide", C);
    const int blocks = ln_bwd_blocks(rows, C);
    const bool posted = post.colscale || post.rowscale;      // the column sums need the finish kernel: summed here, not by the deferred queue
    const size_t need = (size_t)blocks * 2 * C * sizeof(float) + (posted ? (size_t)2 * C * sizeof(float) : 0);
    ISEG_NEED_WORKSPACE("iseg_layernorm_bwd", ws, ws_bytes, need);
    RowReduce red{.P = blocks, .pstride = 2 * C, .n = 2 * C, .out0 = dgamma, .out1 = dbeta, .n0 = C, .accumulate = accumulate_param_grads};
    float* const partials = reduce_rows_begin(red, ws, stream, !posted);      // (see common.h: deferred reductions)
    const size_t lds = 2 * (size_t)C * sizeof(float);
    const int cpl = (C / 8 + lpr - 1) / lpr;
    const int rc = by_dtype(dtype, "iseg_layernorm_bwd", [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto chunks, auto unroll) {
            constexpr int CPL = decltype(chunks)::value, U = decltype(unroll)::value;
            hipLaunchKernelGGL((posted ? layernorm_bwd_kernel<T, CPL, U, true> : layernorm_bwd_kernel<T, CPL, U, false>), dim3(blocks), dim3(256), lds,
                               stream, (const T*)dy, (const T*)x, gamma, mean, rstd, (T*)dx, (const T*)dx_add, partials, rows, C, lpr, dy_index, post);
        };
        // rows in flight per lane group: 4 when a wavefront holds one or two rows per iteration, 2 for four, else 1 (64 / lpr rows already)
        if (cpl <= 1) {
            if (lpr >= 32) launch(IntC<1>{}, IntC<4>{});
            else if (lpr >= 16) launch(IntC<1>{}, IntC<2>{});
            else launch(IntC<1>{}, IntC<1>{});
        } else if (cpl <= 2) launch(IntC<2>{}, IntC<4>{});
        else if (cpl <= 4) launch(IntC<4>{}, IntC<2>{});
        else launch(IntC<8>{}, IntC<1>{});
    });
    if (rc != ISEG_OK) return rc;
    if (posted) {
        float* sums = partials + (size_t)blocks * 2 * C;
        launch_reduce_rows({.partials = partials, .P = blocks, .pstride = 2 * C, .n = 2 * C, .out0 = sums, .n0 = 2 * C}, stream);
        hipLaunchKernelGGL(ln_post_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, sums, post.colscale, gamma, beta, dgamma, dbeta,
                           dcolscale, C);
    } else reduce_rows_end(red, stream);
    return iseg_check_launch("iseg_layernorm_bwd");
}

// LDS of the two BatchNorm reduction kernels: one [2][C] slab row per row lane of the workgroup
static size_t bn_slab_bytes(int C) {
    const int nchunks = C / 8;
    const int tpc = nchunks < 256 ? nchunks : 256;
    return (size_t)(256 / tpc) * 2 * C * sizeof(float);
}

// workgroups of the two reduction kernels.  Measured on [16,128,128,256] bf16 from HBM (tools/kbench_stream.py cold): the statistics pass (one
// tensor, eight rows in flight per lane) is fastest with one workgroup per CU (26.8 us; 38.8 at 1024), the backward sums (three tensors, four
// rows in flight) with four (77.4 us; 102.3 at 256).
static int bn_blocks(int64_t rows, int C, int cap = 256) {
    const int nchunks = C / 8;
    const int tpc = nchunks < 256 ? nchunks : 256;
    const int rpi = 256 / tpc;
    return (int)grid_cap(rows, (int64_t)rpi * 4, cap);
}
constexpr int BN_BWD_REDUCE_MAX_BLOCKS = 1024;

// grid of the element-wise BatchNorm kernels (BnStrip): about eight rows per thread, at most 4096 workgroups
static int bn_strip_blocks(int64_t rows, int C) {
    const int nchunks = C / 8;
    const int tpc = nchunks < 256 ? nchunks : 256;
    const int rpi = 256 / tpc;
    return (int)grid_cap(rows, (int64_t)rpi * 8, 4096);
}

extern "C" size_t iseg_bn_workspace_bytes(int64_t rows, int C) { return (size_t)bn_blocks(rows, C, BN_BWD_REDUCE_MAX_BLOCKS) * 2 * C * sizeof(float); }

extern "C" int iseg_bn_stats(const void* x, int64_t ldx, float* packed, int64_t rows, int C, int dtype, void* ws,
                             size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && packed, "iseg_bn_stats: null pointer");
    ISEG_REQUIRE(rows > 0 && C > 0 && C % 8 == 0 && ldx % 8 == 0, "iseg_bn_stats: C=%d ldx=%lld must be multiples of 8", C,
                 (long long)ldx);
    const int blocks = bn_blocks(rows, C);
    // (the statistics pass runs at most 256 workgroups, the backward sums 1024: the caller is held to the one query that serves both)
    const size_t need = iseg_bn_workspace_bytes(rows, C);
    ISEG_NEED_WORKSPACE("iseg_bn_stats", ws, ws_bytes, need);
    const size_t lds = bn_slab_bytes(C);
    const int rc = by_dtype(dtype, "iseg_bn_stats", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_stats_kernel<T>), dim3(blocks), dim3(256), lds, stream, (const T*)x, ldx, (float*)ws, rows, C, packed + 2 * C);
    });
    if (rc != ISEG_OK) return rc;
    launch_reduce_rows({.partials = (const float*)ws, .P = blocks, .pstride = 2 * C, .n = 2 * C, .out0 = packed, .n0 = 2 * C}, stream);
    return iseg_check_launch("iseg_bn_stats");
}

extern "C" int iseg_bn_finalize(const float* packed, int C, float eps, float momentum, float* mean, float* rstd,
                                float* moving_mean, float* moving_var, hipStream_t stream) {
    ISEG_REQUIRE(packed && mean && rstd && C > 0, "iseg_bn_finalize: bad arguments");
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, packed, C, eps, momentum, mean, rstd,
                       moving_mean, moving_var);
    return iseg_check_launch("iseg_bn_finalize");
}

extern "C" int iseg_bn_apply_fwd(const void* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, void* y, int64_t ldy, int64_t rows, int C, int relu, int dtype,
                                 hipStream_t stream) {
    ISEG_REQUIRE(x && mean && rstd && gamma && beta && y, "iseg_bn_apply_fwd: null pointer");
    ISEG_REQUIRE(C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "iseg_bn_apply_fwd: C/ldx/ldy must be multiples of 8");
    const int blocks = bn_strip_blocks(rows, C);
    return by_dtype(dtype, "iseg_bn_apply_fwd", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_apply_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, stream, (const T*)x, ldx, mean, rstd, gamma, beta, (T*)y, ldy,
                           rows, C, relu);
        return iseg_check_launch("iseg_bn_apply_fwd");
    });
}

extern "C" int iseg_bn_apply_fwd_packed(const void* x, int64_t ldx, const float* packed, float eps, float momentum, const float* gamma,
                                        const float* beta, float* mean, float* rstd, float* moving_mean, float* moving_var, void* y, int64_t ldy,
                                        int64_t rows, int C, int relu, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(x && packed && gamma && beta && mean && rstd && y && rows > 0, "iseg_bn_apply_fwd_packed: bad arguments");
    ISEG_REQUIRE(C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "iseg_bn_apply_fwd_packed: C/ldx/ldy must be multiples of 8");
    ISEG_REQUIRE((((uintptr_t)packed | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)moving_mean | (uintptr_t)moving_var) & 15) == 0,
                 "iseg_bn_apply_fwd_packed: statistics must be 16-byte aligned");
    const int blocks = bn_strip_blocks(rows, C);
    return by_dtype(dtype, "iseg_bn_apply_fwd_packed", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_apply_packed_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, stream, (const T*)x, ldx, packed, eps, momentum, gamma,
                           beta, mean, rstd, moving_mean, moving_var, (T*)y, ldy, rows, C, relu);
        return iseg_check_launch("iseg_bn_apply_fwd_packed");
    });
}

static int bn_bwd_reduce_launch(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                                const float* rstd, const float* re_gamma, const float* re_beta, float* sums, int64_t rows, int C, int relu, int dtype,
                                void* ws, size_t ws_bytes, hipStream_t stream);

extern "C" int iseg_bn_bwd_reduce(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy,
                                  const float* mean, const float* rstd, float* sums, int64_t rows, int C, int relu, int dtype,
                                  void* ws, size_t ws_bytes, hipStream_t stream) {
    return bn_bwd_reduce_launch(dy, lddy, x, ldx, y, ldy, mean, rstd, nullptr, nullptr, sums, rows, C, relu, dtype, ws, ws_bytes, stream);
}

extern "C" int iseg_bn_bwd_reduce_remask(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean, const float* rstd,
                                         const float* gamma, const float* beta, float* sums, int64_t rows, int C, int dtype, void* ws,
                                         size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(gamma && beta && (((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, "iseg_bn_bwd_reduce_remask: gamma / beta must be 16-byte aligned");
    return bn_bwd_reduce_launch(dy, lddy, x, ldx, nullptr, 0, mean, rstd, gamma, beta, sums, rows, C, 1, dtype, ws, ws_bytes, stream);
}

static int bn_bwd_reduce_launch(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                                const float* rstd, const float* re_gamma, const float* re_beta, float* sums, int64_t rows, int C, int relu, int dtype,
                                void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(dy && x && mean && rstd && sums && (!relu || y || re_gamma), "iseg_bn_bwd_reduce: null pointer");
    ISEG_REQUIRE(C % 8 == 0 && ldx % 8 == 0 && lddy % 8 == 0 && (!relu || re_gamma || ldy % 8 == 0), "iseg_bn_bwd_reduce: alignment");
    const int blocks = bn_blocks(rows, C, BN_BWD_REDUCE_MAX_BLOCKS);
    const size_t need = (size_t)blocks * 2 * C * sizeof(float);
    ISEG_NEED_WORKSPACE("iseg_bn_bwd_reduce", ws, ws_bytes, need);
    const size_t lds = bn_slab_bytes(C);
    const int rc = by_dtype(dtype, "iseg_bn_bwd_reduce", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<T>), dim3(blocks), dim3(256), lds, stream, (const T*)dy, lddy, (const T*)x, ldx, (const T*)y, ldy,
                           mean, rstd, (float*)ws, rows, C, relu, re_gamma, re_beta);
    });
    if (rc != ISEG_OK) return rc;
    launch_reduce_rows({.partials = (const float*)ws, .P = blocks, .pstride = 2 * C, .n = 2 * C, .out0 = sums, .n0 = 2 * C}, stream);
    return iseg_check_launch("iseg_bn_bwd_reduce");
}

extern "C" int iseg_bn_bwd_apply_acc(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy,
                                     const float* mean, const float* rstd, const float* gamma, const float* sums, float inv_n,
                                     void* dx, int64_t lddx, float* dgamma, float* dbeta, int64_t rows, int C, int relu, int dtype,
                                     hipStream_t stream);

extern "C" int iseg_bn_bwd_apply(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy,
                                 const float* mean, const float* rstd, const float* gamma, const float* sums, float inv_n,
                                 void* dx, int64_t lddx, int64_t rows, int C, int relu, int dtype, hipStream_t stream) {
    return iseg_bn_bwd_apply_acc(dy, lddy, x, ldx, y, ldy, mean, rstd, gamma, sums, inv_n, dx, lddx, nullptr, nullptr, rows, C, relu, dtype, stream);
}

static int bn_bwd_apply_launch(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                               const float* rstd, const float* gamma, const float* re_beta, const float* sums, float inv_n, void* dx, int64_t lddx,
                               float* dgamma, float* dbeta, int64_t rows, int C, int relu, int dtype, hipStream_t stream);

extern "C" int iseg_bn_bwd_apply_acc(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy,
                                     const float* mean, const float* rstd, const float* gamma, const float* sums, float inv_n,
                                     void* dx, int64_t lddx, float* dgamma, float* dbeta, int64_t rows, int C, int relu, int dtype,
                                     hipStream_t stream) {
    return bn_bwd_apply_launch(dy, lddy, x, ldx, y, ldy, mean, rstd, gamma, nullptr, sums, inv_n, dx, lddx, dgamma, dbeta, rows, C, relu, dtype, stream);
}

extern "C" int iseg_bn_bwd_apply_remask(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean, const float* rstd,
                                        const float* gamma, const float* beta, const float* sums, float inv_n, void* dx, int64_t lddx,
                                        float* dgamma, float* dbeta, int64_t rows, int C, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(beta && ((uintptr_t)beta & 15) == 0, "iseg_bn_bwd_apply_remask: beta must be 16-byte aligned");
    return bn_bwd_apply_launch(dy, lddy, x, ldx, nullptr, 0, mean, rstd, gamma, beta, sums, inv_n, dx, lddx, dgamma, dbeta, rows, C, 1, dtype, stream);
}

static int bn_bwd_apply_launch(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                               const float* rstd, const float* gamma, const float* re_beta, const float* sums, float inv_n, void* dx, int64_t lddx,
                               float* dgamma, float* dbeta, int64_t rows, int C, int relu, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(dy && x && mean && rstd && gamma && sums && dx && (!relu || y || re_beta), "iseg_bn_bwd_apply: null pointer");
    ISEG_REQUIRE(C % 8 == 0 && ldx % 8 == 0 && lddy % 8 == 0 && lddx % 8 == 0, "iseg_bn_bwd_apply: alignment");
    ISEG_REQUIRE((((uintptr_t)dgamma | (uintptr_t)dbeta) & 15) == 0 && (!(dgamma || dbeta) || ((uintptr_t)sums & 15) == 0),
                 "iseg_bn_bwd_apply_acc: gradient vectors must be 16-byte aligned");
    const int blocks = bn_strip_blocks(rows, C);
    return by_dtype(dtype, "iseg_bn_bwd_apply", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, stream, (const T*)dy, lddy, (const T*)x, ldx, (const T*)y,
                           ldy, mean, rstd, gamma, sums, inv_n, (T*)dx, lddx, rows, C, relu, dgamma, dbeta, re_beta);
        return iseg_check_launch("iseg_bn_bwd_apply");
    });
}
