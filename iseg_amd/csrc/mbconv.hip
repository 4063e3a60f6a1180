// The BN -> swish -> squeeze-excite -> gate tail of an EfficientNet MBConv block (reference backbones/efficientnet.py:214-255) on the
// depthwise output x [N, H, W, C] (NHWC; the rows of sample n are [n*HW, (n+1)*HW)):
//
//   z = (x - mean) * rstd * gamma + beta,   a = swish(z) = z * sigmoid(z)
//   m[n, c] = mean_hw a,   h = swish(W1^T m + b1) [N, Cse],   g = sigmoid(W2^T h + b2) [N, C],   out = a * g
//
// The un-gated a is never written.  Forward: squeeze pass (reads x, writes per-(n, part, c) partial sums), excite launch (the SE MLP of all
// samples, fp32), gate pass (reads x, writes out).  Backward with dO = d out, s' = swish'(z), xhat = (x - mean) * rstd:
//   reduce pass: per (n, part, c)  S1 = sum dO*a, S2 = sum dO*s', S3 = sum dO*s'*xhat, S4 = sum s', S5 = sum s'*xhat
//   excite backward (three grid-wide launches: part sums; per-sample MLP backward; sample-ordered parameter / BatchNorm sums):
//       dg = S1 -> dW2, db2, dh -> dW1, db1, dm;  with da = dO*g + dm/HW and dz = da*s' the BatchNorm sums
//       sums[0:C] = sum dz = sum_n (g*S2 + dm/HW*S4),   sums[C:2C] = sum dz*xhat = sum_n (g*S3 + dm/HW*S5)   (iseg_bn_bwd_reduce's layout)
//   apply pass: dx = gamma*rstd*(dz - sums0/cnt - xhat*sums1/cnt) (training statistics) or gamma*rstd*dz (moving statistics).
//
// Streaming passes: one lane owns eight consecutive channels of a row (16-byte bf16 / 2 x 16-byte fp32 accesses); a 256-lane workgroup
// tiles (sample, row part, channel slab of <= 512 channels).  Partial sums of a workgroup are combined through LDS in row-lane order and
// written to the caller's buffer; every later sum runs in a fixed order, and there are no floating-point atomics: results are bitwise
// reproducible.  Storage fp32 or bf16, arithmetic fp32; C % 8 == 0, any H*W, any Cse >= 1.
#include "common.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_SLAB_CHUNKS = 64;      // eight-channel chunks per workgroup slab (512 channels)
constexpr int MB_MAX_PARTS = 64;        // row parts per sample
constexpr int MBX_THREADS = 1024;       // the excite forward (one workgroup per sample)

struct MbTile {
    int nchunks, tpc, rpi, slabs, parts;
    int64_t rows_per_part;
};

// Depends on the shape only, so the summation order (and the result bits) is a function of the shape.
MbTile mb_tile(int HW, int C) {
    MbTile t;
    t.nchunks = C / 8;
    t.tpc = t.nchunks < MB_SLAB_CHUNKS ? t.nchunks : MB_SLAB_CHUNKS;
    t.rpi = MB_THREADS / t.tpc;
    t.slabs = (t.nchunks + t.tpc - 1) / t.tpc;
    int64_t parts = ceil_div64(HW, (int64_t)t.rpi * 8);      // about eight rows per lane
    if (parts > MB_MAX_PARTS) parts = MB_MAX_PARTS;
    if (parts < 1) parts = 1;
    t.rows_per_part = ceil_div64(HW, parts);
    t.parts = (int)ceil_div64(HW, t.rows_per_part);      // no empty part
    return t;
}

__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

// Lane geometry of a streaming pass: channel chunk `cc` (global), row lane `tr`, rows [r0, r1) of sample blockIdx.z.
struct MbLane {
    int tc, tr, cc;
    bool active;
    int64_t r0, r1;
    __device__ MbLane(int nchunks, int tpc, int rpi, int64_t HW, int64_t rows_per_part) {
        tc = threadIdx.x % tpc;
        tr = threadIdx.x / tpc;
        cc = blockIdx.y * tpc + tc;
        active = tr < rpi && cc < nchunks;
        r0 = (int64_t)blockIdx.x * rows_per_part;
        r1 = r0 + rows_per_part < HW ? r0 + rows_per_part : HW;
    }
};

template <class T>
__device__ __forceinline__ void mb_load_consts(const float* mean, const float* rstd, const float* gamma, const float* beta, int c,
                                               float* m, float* rs, float* g, float* b) {
    load8<float>(mean + c, m);
    load8<float>(rstd + c, rs);
    load8<float>(gamma + c, g);
    load8<float>(beta + c, b);
}

// NQ quantities per (n, part, c): lanes of one chunk put theirs in LDS [row lane][q][slab channel]; the first 8*tpc*NQ lanes sum them in
// row-lane order and write partials[((n * parts + part) * NQ + q) * C + c].
template <int NQ>
__device__ __forceinline__ void mb_flush(float (*acc)[8], const MbLane& L, int tpc, int rpi, int C, int parts, float* __restrict__ partials,
                                         float* lds) {
    const int sw = tpc * 8;
    if (L.tr < rpi) {      // lanes past the last chunk store zeros: every read cell is written
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int u = 0; u < 8; ++u) lds[((size_t)L.tr * NQ + q) * sw + L.tc * 8 + u] = L.active ? acc[q][u] : 0.f;
    }
    __syncthreads();
    const int cbase = blockIdx.y * sw;
    float* out = partials + ((int64_t)blockIdx.z * parts + blockIdx.x) * NQ * C;
    for (int i = threadIdx.x; i < NQ * sw; i += MB_THREADS) {
        const int q = i / sw, j = i % sw;
        if (cbase + j >= C) continue;
        float s = 0.f;
        for (int t = 0; t < rpi; ++t) s += lds[((size_t)t * NQ + q) * sw + j];
        out[(int64_t)q * C + cbase + j] = s;
    }
}

template <class T>
__global__ __launch_bounds__(MB_THREADS) void mb_squeeze_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ partials, int HW, int C,
                                                                MbTile t) {
    __shared__ __attribute__((aligned(16))) float lds[MB_THREADS * 8];
    const MbLane L(t.nchunks, t.tpc, t.rpi, HW, t.rows_per_part);
    float acc[1][8] = {};
    if (L.active) {
        const int c = L.cc * 8;
        float m[8], rs[8], g[8], b[8];
        mb_load_consts<T>(mean, rstd, gamma, beta, c, m, rs, g, b);
        const T* xs = x + (int64_t)blockIdx.z * HW * C + c;
        int64_t r = L.r0 + L.tr;
        constexpr int UB = 4;
        for (; r + (UB - 1) * t.rpi < L.r1; r += UB * t.rpi) {
            float v[UB][8];
#pragma unroll
            for (int k = 0; k < UB; ++k) load8<T>(xs + (r + k * t.rpi) * C, v[k]);
#pragma unroll
            for (int k = 0; k < UB; ++k)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float z = (v[k][u] - m[u]) * rs[u] * g[u] + b[u];
                    acc[0][u] += z * sigm(z);
                }
        }
        for (; r < L.r1; r += t.rpi) {
            float v[8];
            load8<T>(xs + r * C, v);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float z = (v[u] - m[u]) * rs[u] * g[u] + b[u];
                acc[0][u] += z * sigm(z);
            }
        }
    }
    mb_flush<1>(acc, L, t.tpc, t.rpi, C, t.parts, partials, lds);
}

template <class T>
__global__ __launch_bounds__(MB_THREADS) void mb_gate_fwd_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ gate,
                                                                 T* __restrict__ out, int HW, int C, MbTile t) {
    const MbLane L(t.nchunks, t.tpc, t.rpi, HW, t.rows_per_part);
    if (!L.active) return;
    const int c = L.cc * 8;
    float m[8], rs[8], g[8], b[8], s[8];
    mb_load_consts<T>(mean, rstd, gamma, beta, c, m, rs, g, b);
    load8<float>(gate + (int64_t)blockIdx.z * C + c, s);
    const int64_t base = (int64_t)blockIdx.z * HW * C + c;
    int64_t r = L.r0 + L.tr;
    constexpr int UB = 4;
    for (; r + (UB - 1) * t.rpi < L.r1; r += UB * t.rpi) {
        float v[UB][8];
#pragma unroll
        for (int k = 0; k < UB; ++k) load8<T>(x + base + (r + k * t.rpi) * C, v[k]);
#pragma unroll
        for (int k = 0; k < UB; ++k) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float z = (v[k][u] - m[u]) * rs[u] * g[u] + b[u];
                v[k][u] = z * sigm(z) * s[u];
            }
            store8<T>(out + base + (r + k * t.rpi) * C, v[k]);
        }
    }
    for (; r < L.r1; r += t.rpi) {
        float v[8];
        load8<T>(x + base + r * C, v);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float z = (v[u] - m[u]) * rs[u] * g[u] + b[u];
            v[u] = z * sigm(z) * s[u];
        }
        store8<T>(out + base + r * C, v);
    }
}

// z, a = swish(z), s' = swish'(z) = sigmoid(z) * (1 + z * (1 - sigmoid(z))), xhat of one element
struct MbElem {
    float xh, a, sp;
    __device__ __forceinline__ MbElem(float v, float m, float rs, float g, float b) {
        xh = (v - m) * rs;
        const float z = xh * g + b;
        const float sg = sigm(z);
        a = z * sg;
        sp = sg * (1.f + z * (1.f - sg));
    }
};

template <class T>
__global__ __launch_bounds__(MB_THREADS) void mb_bwd_reduce_kernel(const T* __restrict__ dO, const T* __restrict__ x,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float* __restrict__ partials, int HW, int C, MbTile t) {
    __shared__ __attribute__((aligned(16))) float lds[5 * MB_THREADS * 8];
    const MbLane L(t.nchunks, t.tpc, t.rpi, HW, t.rows_per_part);
    float acc[5][8] = {};
    if (L.active) {
        const int c = L.cc * 8;
        float m[8], rs[8], g[8], b[8];
        mb_load_consts<T>(mean, rstd, gamma, beta, c, m, rs, g, b);
        const int64_t base = (int64_t)blockIdx.z * HW * C + c;
        int64_t r = L.r0 + L.tr;
        constexpr int UB = 2;
        for (; r + (UB - 1) * t.rpi < L.r1; r += UB * t.rpi) {
            float v[UB][8], d[UB][8];
#pragma unroll
            for (int k = 0; k < UB; ++k) {
                load8<T>(x + base + (r + k * t.rpi) * C, v[k]);
                load8<T>(dO + base + (r + k * t.rpi) * C, d[k]);
            }
#pragma unroll
            for (int k = 0; k < UB; ++k)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const MbElem e(v[k][u], m[u], rs[u], g[u], b[u]);
                    const float ds = d[k][u] * e.sp;
                    acc[0][u] += d[k][u] * e.a;
                    acc[1][u] += ds;
                    acc[2][u] += ds * e.xh;
                    acc[3][u] += e.sp;
                    acc[4][u] += e.sp * e.xh;
                }
        }
        for (; r < L.r1; r += t.rpi) {
            float v[8], d[8];
            load8<T>(x + base + r * C, v);
            load8<T>(dO + base + r * C, d);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const MbElem e(v[u], m[u], rs[u], g[u], b[u]);
                const float ds = d[u] * e.sp;
                acc[0][u] += d[u] * e.a;
                acc[1][u] += ds;
                acc[2][u] += ds * e.xh;
                acc[3][u] += e.sp;
                acc[4][u] += e.sp * e.xh;
            }
        }
    }
    mb_flush<5>(acc, L, t.tpc, t.rpi, C, t.parts, partials, lds);
}

// dz = (dO * g + dmh) * s';  training: dx = gamma*rstd*(dz - sums0*inv_n - xhat*sums1*inv_n);  moving statistics: dx = gamma*rstd*dz.
// dbeta += sums[0:C], dgamma += sums[C:2C] (either may be null) by the lanes of row part 0 of sample 0.
template <class T>
__global__ __launch_bounds__(MB_THREADS) void mb_bwd_apply_kernel(const T* __restrict__ dO, const T* __restrict__ x,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ gate, const float* __restrict__ dmh,
                                                                  const float* __restrict__ sums, float inv_n, int train,
                                                                  T* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  int HW, int C, MbTile t) {
    const MbLane L(t.nchunks, t.tpc, t.rpi, HW, t.rows_per_part);
    if (!L.active) return;
    const int c = L.cc * 8;
    float m[8], rs[8], g[8], b[8], s1[8], s2[8], gt[8], dh[8];
    mb_load_consts<T>(mean, rstd, gamma, beta, c, m, rs, g, b);
    load8<float>(sums + c, s1);
    load8<float>(sums + C + c, s2);
    load8<float>(gate + (int64_t)blockIdx.z * C + c, gt);
    load8<float>(dmh + (int64_t)blockIdx.z * C + c, dh);
    if (blockIdx.x == 0 && blockIdx.z == 0 && L.tr == 0) {
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
    const float tr = train ? inv_n : 0.f;
    const int64_t base = (int64_t)blockIdx.z * HW * C + c;
    int64_t r = L.r0 + L.tr;
    constexpr int UB = 2;
    for (; r + (UB - 1) * t.rpi < L.r1; r += UB * t.rpi) {
        float v[UB][8], d[UB][8];
#pragma unroll
        for (int k = 0; k < UB; ++k) {
            load8<T>(x + base + (r + k * t.rpi) * C, v[k]);
            load8<T>(dO + base + (r + k * t.rpi) * C, d[k]);
        }
#pragma unroll
        for (int k = 0; k < UB; ++k) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const MbElem e(v[k][u], m[u], rs[u], g[u], b[u]);
                const float dz = (d[k][u] * gt[u] + dh[u]) * e.sp;
                d[k][u] = g[u] * rs[u] * (dz - s1[u] * tr - e.xh * s2[u] * tr);
            }
            store8<T>(dx + base + (r + k * t.rpi) * C, d[k]);
        }
    }
    for (; r < L.r1; r += t.rpi) {
        float v[8], d[8];
        load8<T>(x + base + r * C, v);
        load8<T>(dO + base + r * C, d);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const MbElem e(v[u], m[u], rs[u], g[u], b[u]);
            const float dz = (d[u] * gt[u] + dh[u]) * e.sp;
            d[u] = g[u] * rs[u] * (dz - s1[u] * tr - e.xh * s2[u] * tr);
        }
        store8<T>(dx + base + r * C, d);
    }
}

// Excite, one workgroup per sample: m = (sum of the part partials in part order) / HW, hpre = W1^T m + b1 (one wavefront per output, lanes
// over C, fixed-order lane sum), g = sigmoid(W2^T swish(hpre) + b2).  W1 [C, Cse], W2 [Cse, C] (Keras 1 x 1 kernels).  LDS: m [C], h [Cse].
__global__ __launch_bounds__(MBX_THREADS) void mb_excite_fwd_kernel(const float* __restrict__ partials, int parts, int HW, int C, int Cse,
                                                                    const float* __restrict__ W1, const float* __restrict__ b1,
                                                                    const float* __restrict__ W2, const float* __restrict__ b2,
                                                                    float* __restrict__ m_out, float* __restrict__ hpre_out,
                                                                    float* __restrict__ g_out) {
    extern __shared__ __attribute__((aligned(16))) float xl[];
    float* lm = xl;
    float* lh = xl + C;
    const int n = blockIdx.x;
    const float inv_hw = 1.f / (float)HW;
    for (int c = threadIdx.x; c < C; c += MBX_THREADS) {
        float s = 0.f;
        for (int p = 0; p < parts; ++p) s += partials[((int64_t)n * parts + p) * C + c];
        const float mv = s * inv_hw;
        lm[c] = mv;
        m_out[(int64_t)n * C + c] = mv;
    }
    __syncthreads();
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int j = wave; j < Cse; j += MBX_THREADS / 64) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += W1[(int64_t)c * Cse + j] * lm[c];
        s = wave_sum(s);
        if (lane == 0) {
            const float pre = s + b1[j];
            hpre_out[(int64_t)n * Cse + j] = pre;
            lh[j] = pre * sigm(pre);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += MBX_THREADS) {
        float e = b2[c];
        for (int j = 0; j < Cse; ++j) e += W2[(int64_t)j * C + c] * lh[j];
        g_out[(int64_t)n * C + c] = sigm(e);
    }
}

// Excite backward in three launches, each spread over the whole chip; every sum runs in a fixed order (no float atomics).  Scratch (ws):
// S [N][5][C] (the part sums of the reduce pass), de [N][C] (gradient of the pre-sigmoid excite), dh [N][Cse] (of the pre-swish squeeze).
constexpr int MBB_THREADS = 256;

// 1. one lane per (n, q, c): S = sum over the row parts in part order (four interleaved chains, combined as (c0 + c1) + (c2 + c3));
//    the lanes of q = 0 also form de = S1 * g * (1 - g)   (dg = S1).
__global__ __launch_bounds__(MBB_THREADS) void mb_excite_bwd_parts_kernel(const float* __restrict__ partials, int parts, int N, int C,
                                                                          const float* __restrict__ gate, float* __restrict__ S,
                                                                          float* __restrict__ de) {
    const int64_t i = (int64_t)blockIdx.x * MBB_THREADS + threadIdx.x;
    if (i >= (int64_t)N * 5 * C) return;
    const int c = (int)(i % C), q = (int)((i / C) % 5), n = (int)(i / ((int64_t)5 * C));
    const float* src = partials + ((int64_t)n * parts * 5 + q) * C + c;
    const int64_t ps = (int64_t)5 * C;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int p = 0;
    for (; p + 3 < parts; p += 4) {
        a0 += src[(p + 0) * ps];
        a1 += src[(p + 1) * ps];
        a2 += src[(p + 2) * ps];
        a3 += src[(p + 3) * ps];
    }
    for (; p < parts; ++p) a0 += src[p * ps];
    const float s = (a0 + a1) + (a2 + a3);
    S[i] = s;
    if (q == 0) {
        const float gv = gate[(int64_t)n * C + c];
        de[(int64_t)n * C + c] = s * gv * (1.f - gv);
    }
}

// 2. one workgroup per sample: dh[n, j] = swish'(hpre[n, j]) * sum_c W2[j, c] de[n, c]  (a wavefront per j, lanes over c, fixed-order lane
//    sum), then dmh[n, c] = sum_j W1[c, j] dh[n, j] / HW.  LDS: dh of the sample [Cse].
__global__ __launch_bounds__(MBB_THREADS) void mb_excite_bwd_sample_kernel(int HW, int C, int Cse, const float* __restrict__ W1,
                                                                           const float* __restrict__ W2, const float* __restrict__ hpre,
                                                                           const float* __restrict__ de, float* __restrict__ dh,
                                                                           float* __restrict__ dmh) {
    extern __shared__ __attribute__((aligned(16))) float ldh[];
    const int n = blockIdx.x;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const float* den = de + (int64_t)n * C;
    for (int j = wave; j < Cse; j += MBB_THREADS / 64) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += W2[(int64_t)j * C + c] * den[c];
        s = wave_sum(s);
        if (lane == 0) {
            const float pre = hpre[(int64_t)n * Cse + j], sg = sigm(pre);
            const float v = s * sg * (1.f + pre * (1.f - sg));
            ldh[j] = v;
            dh[(int64_t)n * Cse + j] = v;
        }
    }
    __syncthreads();
    const float inv_hw = 1.f / (float)HW;
    for (int c = threadIdx.x; c < C; c += MBB_THREADS) {
        float s = 0.f;
        const float* w = W1 + (int64_t)c * Cse;
        for (int j = 0; j < Cse; ++j) s += w[j] * ldh[j];
        dmh[(int64_t)n * C + c] = s * inv_hw;
    }
}

// 3. one lane per output, each summing over the samples in order n = 0..N-1:
//    [0, Cse*C)        dW2[j, c] (+)= sum_n swish(hpre[n, j]) * de[n, c]
//    [.., +C)          db2[c]    (+)= sum_n de[n, c]
//    [.., +C*Cse)      dW1[c, j] (+)= sum_n m[n, c] * dh[n, j]
//    [.., +Cse)        db1[j]    (+)= sum_n dh[n, j]
//    [.., +C)          sums[c] = sum_n (g*S2 + dmh*S4),  sums[C + c] = sum_n (g*S3 + dmh*S5)
__global__ __launch_bounds__(MBB_THREADS) void mb_excite_bwd_sums_kernel(int N, int C, int Cse, const float* __restrict__ m,
                                                                         const float* __restrict__ hpre, const float* __restrict__ gate,
                                                                         const float* __restrict__ S, const float* __restrict__ de,
                                                                         const float* __restrict__ dh, const float* __restrict__ dmh,
                                                                         float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
                                                                         float* __restrict__ db2, int accumulate, float* __restrict__ sums) {
    int64_t i = (int64_t)blockIdx.x * MBB_THREADS + threadIdx.x;
    const int64_t CseC = (int64_t)Cse * C;
    if (i < CseC) {
        const int j = (int)(i / C), c = (int)(i % C);
        float s = 0.f;
        for (int n = 0; n < N; ++n) {
            const float pre = hpre[(int64_t)n * Cse + j];
            s += pre * sigm(pre) * de[(int64_t)n * C + c];
        }
        if (dW2) dW2[i] = accumulate ? dW2[i] + s : s;
        return;
    }
    i -= CseC;
    if (i < C) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += de[(int64_t)n * C + i];
        if (db2) db2[i] = accumulate ? db2[i] + s : s;
        return;
    }
    i -= C;
    if (i < CseC) {
        const int c = (int)(i / Cse), j = (int)(i % Cse);
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += m[(int64_t)n * C + c] * dh[(int64_t)n * Cse + j];
        if (dW1) dW1[i] = accumulate ? dW1[i] + s : s;
        return;
    }
    i -= CseC;
    if (i < Cse) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += dh[(int64_t)n * Cse + i];
        if (db1) db1[i] = accumulate ? db1[i] + s : s;
        return;
    }
    i -= Cse;
    if (i < C) {
        float s0 = 0.f, s1 = 0.f;
        for (int n = 0; n < N; ++n) {
            const float gv = gate[(int64_t)n * C + i], dv = dmh[(int64_t)n * C + i];
            const float* Sn = S + (int64_t)n * 5 * C + i;
            s0 += gv * Sn[C] + dv * Sn[3 * (int64_t)C];
            s1 += gv * Sn[2 * (int64_t)C] + dv * Sn[4 * (int64_t)C];
        }
        sums[i] = s0;
        sums[C + i] = s1;
    }
}

constexpr size_t MBX_MAX_LDS = 64 * 1024;

bool mb_shape_ok(int N, int HW, int C, int Cse) {
    return N > 0 && HW > 0 && C > 0 && C % 8 == 0 && Cse >= 1 && (size_t)(C + Cse) * sizeof(float) <= MBX_MAX_LDS;
}

bool mb_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define MB_UNSUPPORTED(what, N, HW, C, Cse)                                                                                  \
    do {                                                                                                                     \
        iseg_set_error("%s: unsupported shape N=%d HW=%d C=%d Cse=%d (C %% 8 == 0, 16-byte aligned tensors)", what, N, HW, C, \
                       Cse);                                                                                                 \
        return ISEG_ERR_UNSUPPORTED;                                                                                         \
    } while (0)

}  // namespace

extern "C" int iseg_mbconv_supported(int N, int HW, int C, int Cse) { return mb_shape_ok(N, HW, C, Cse) ? 1 : 0; }

extern "C" size_t iseg_mbconv_partials_bytes(int N, int HW, int C, int backward) {
    if (!mb_shape_ok(N, HW, C, 1)) return 0;
    const MbTile t = mb_tile(HW, C);
    return (size_t)N * t.parts * (backward ? 5 : 1) * C * sizeof(float);
}

extern "C" size_t iseg_se_excite_bwd_workspace_bytes(int N, int C, int Cse) { return ((size_t)N * 6 * C + (size_t)N * Cse) * sizeof(float); }

extern "C" int iseg_bn_swish_se_squeeze(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                        float* partials, size_t partials_bytes, int N, int HW, int C, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(x && mean && rstd && gamma && beta && partials, "iseg_bn_swish_se_squeeze: null pointer");
    if (!mb_shape_ok(N, HW, C, 1) || !mb_aligned(x) || !mb_aligned(mean) || !mb_aligned(rstd) || !mb_aligned(gamma) || !mb_aligned(beta))
        MB_UNSUPPORTED("iseg_bn_swish_se_squeeze", N, HW, C, 0);
    ISEG_REQUIRE(partials_bytes >= iseg_mbconv_partials_bytes(N, HW, C, 0), "iseg_bn_swish_se_squeeze: partials buffer too small");
    const MbTile t = mb_tile(HW, C);
    const dim3 grid(t.parts, t.slabs, N);
    return by_dtype(dtype, "iseg_bn_swish_se_squeeze", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(mb_squeeze_kernel<T>, grid, dim3(MB_THREADS), 0, stream, (const T*)x, mean, rstd, gamma, beta, partials, HW, C, t);
        return iseg_check_launch("iseg_bn_swish_se_squeeze");
    });
}

extern "C" int iseg_se_excite_fwd(const float* partials, int N, int HW, int C, int Cse, const float* W1, const float* b1, const float* W2,
                                  const float* b2, float* m, float* hpre, float* g, hipStream_t stream) {
    ISEG_REQUIRE(partials && W1 && b1 && W2 && b2 && m && hpre && g, "iseg_se_excite_fwd: null pointer");
    if (!mb_shape_ok(N, HW, C, Cse)) MB_UNSUPPORTED("iseg_se_excite_fwd", N, HW, C, Cse);
    const MbTile t = mb_tile(HW, C);
    hipLaunchKernelGGL(mb_excite_fwd_kernel, dim3(N), dim3(MBX_THREADS), (C + Cse) * sizeof(float), stream, partials, t.parts, HW, C, Cse, W1,
                       b1, W2, b2, m, hpre, g);
    return iseg_check_launch("iseg_se_excite_fwd");
}

extern "C" int iseg_bn_swish_gate_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                      const float* g, void* out, int N, int HW, int C, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(x && mean && rstd && gamma && beta && g && out, "iseg_bn_swish_gate_fwd: null pointer");
    if (!mb_shape_ok(N, HW, C, 1) || !mb_aligned(x) || !mb_aligned(out) || !mb_aligned(g) || !mb_aligned(mean) || !mb_aligned(rstd) ||
        !mb_aligned(gamma) || !mb_aligned(beta))
        MB_UNSUPPORTED("iseg_bn_swish_gate_fwd", N, HW, C, 0);
    const MbTile t = mb_tile(HW, C);
    const dim3 grid(t.parts, t.slabs, N);
    return by_dtype(dtype, "iseg_bn_swish_gate_fwd", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(mb_gate_fwd_kernel<T>, grid, dim3(MB_THREADS), 0, stream, (const T*)x, mean, rstd, gamma, beta, g, (T*)out, HW, C, t);
        return iseg_check_launch("iseg_bn_swish_gate_fwd");
    });
}

extern "C" int iseg_bn_swish_gate_bwd_reduce(const void* dO, const void* x, const float* mean, const float* rstd, const float* gamma,
                                             const float* beta, float* partials, size_t partials_bytes, int N, int HW, int C, int dtype,
                                             hipStream_t stream) {
    ISEG_REQUIRE(dO && x && mean && rstd && gamma && beta && partials, "iseg_bn_swish_gate_bwd_reduce: null pointer");
    if (!mb_shape_ok(N, HW, C, 1) || !mb_aligned(x) || !mb_aligned(dO) || !mb_aligned(mean) || !mb_aligned(rstd) || !mb_aligned(gamma) ||
        !mb_aligned(beta))
        MB_UNSUPPORTED("iseg_bn_swish_gate_bwd_reduce", N, HW, C, 0);
    ISEG_REQUIRE(partials_bytes >= iseg_mbconv_partials_bytes(N, HW, C, 1), "iseg_bn_swish_gate_bwd_reduce: partials buffer too small");
    const MbTile t = mb_tile(HW, C);
    const dim3 grid(t.parts, t.slabs, N);
    return by_dtype(dtype, "iseg_bn_swish_gate_bwd_reduce", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(mb_bwd_reduce_kernel<T>, grid, dim3(MB_THREADS), 0, stream, (const T*)dO, (const T*)x, mean, rstd, gamma, beta, partials,
                           HW, C, t);
        return iseg_check_launch("iseg_bn_swish_gate_bwd_reduce");
    });
}

extern "C" int iseg_se_excite_bwd(const float* partials, int N, int HW, int C, int Cse, const float* W1, const float* W2, const float* m,
                                  const float* hpre, const float* g, float* dW1, float* db1, float* dW2, float* db2, int accumulate, float* dmh,
                                  float* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(partials && W1 && W2 && m && hpre && g && dmh && sums && ws, "iseg_se_excite_bwd: null pointer");
    if (!mb_shape_ok(N, HW, C, Cse)) MB_UNSUPPORTED("iseg_se_excite_bwd", N, HW, C, Cse);
    ISEG_NEED_WORKSPACE("iseg_se_excite_bwd", ws, ws_bytes, iseg_se_excite_bwd_workspace_bytes(N, C, Cse));
    const MbTile t = mb_tile(HW, C);
    float* S = (float*)ws;
    float* de = S + (int64_t)N * 5 * C;
    float* dh = de + (int64_t)N * C;
    const int64_t nparts = (int64_t)N * 5 * C;
    hipLaunchKernelGGL(mb_excite_bwd_parts_kernel, dim3((unsigned)ceil_div64(nparts, MBB_THREADS)), dim3(MBB_THREADS), 0, stream, partials, t.parts,
                       N, C, g, S, de);
    hipLaunchKernelGGL(mb_excite_bwd_sample_kernel, dim3(N), dim3(MBB_THREADS), Cse * sizeof(float), stream, HW, C, Cse, W1, W2, hpre, de, dh,
                       dmh);
    const int64_t nsums = 2 * (int64_t)Cse * C + 2 * (int64_t)C + Cse;
    hipLaunchKernelGGL(mb_excite_bwd_sums_kernel, dim3((unsigned)ceil_div64(nsums, MBB_THREADS)), dim3(MBB_THREADS), 0, stream, N, C, Cse, m, hpre,
                       g, S, de, dh, dmh, dW1, db1, dW2, db2, accumulate, sums);
    return iseg_check_launch("iseg_se_excite_bwd");
}

extern "C" int iseg_bn_swish_gate_bwd_apply(const void* dO, const void* x, const float* mean, const float* rstd, const float* gamma,
                                            const float* beta, const float* g, const float* dmh, const float* sums, float inv_n, int train,
                                            void* dx, float* dgamma, float* dbeta, int N, int HW, int C, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(dO && x && mean && rstd && gamma && beta && g && dmh && sums && dx, "iseg_bn_swish_gate_bwd_apply: null pointer");
    if (!mb_shape_ok(N, HW, C, 1) || !mb_aligned(x) || !mb_aligned(dO) || !mb_aligned(dx) || !mb_aligned(g) || !mb_aligned(dmh) ||
        !mb_aligned(sums) || !mb_aligned(mean) || !mb_aligned(rstd) || !mb_aligned(gamma) || !mb_aligned(beta) ||
        (dgamma && !mb_aligned(dgamma)) || (dbeta && !mb_aligned(dbeta)))
        MB_UNSUPPORTED("iseg_bn_swish_gate_bwd_apply", N, HW, C, 0);
    const MbTile t = mb_tile(HW, C);
    const dim3 grid(t.parts, t.slabs, N);
    return by_dtype(dtype, "iseg_bn_swish_gate_bwd_apply", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(mb_bwd_apply_kernel<T>, grid, dim3(MB_THREADS), 0, stream, (const T*)dO, (const T*)x, mean, rstd, gamma, beta, g, dmh,
                           sums, inv_n, train, (T*)dx, dgamma, dbeta, HW, C, t);
        return iseg_check_launch("iseg_bn_swish_gate_bwd_apply");
    });
}
