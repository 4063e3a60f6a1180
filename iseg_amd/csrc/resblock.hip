// The residual tail of the ResNet-9 / 10 / 18 basic block (reference backbones/resnet_blocks_small.py, BlockType2Small.call :84-119):
//
//   out = relu( bn2(z2) + pool_s(sc) ),   bn(v) = (v - mean) * rstd * gamma + beta
//   sc  = bn0(z0)   (block with a shortcut conv)   or   x   (identity shortcut)
//   pool_s = tf.nn.avg_pool2d(window = strides = s, "SAME"), s in {1, 2}: padded cells do not count in the divisor (odd H / W give partial
//            last windows).  The shortcut input is [N, H, W, C]; z2 and out are [N, Ho, Wo, C] with Ho = ceil(H / s), Wo = ceil(W / s).
//
// The composed route writes bn2(z2), bn0(z0) and the pooled shortcut before the add; here the forward reads z2 and the shortcut input once
// and writes only out.  Since bn0 is affine per channel, pool(bn0(z0)) = bn0(pool(z0)): the window is averaged first.
//
// Backward, with g = dout * [out > 0] on the output rows and u = unpool(g) / count on the full-resolution rows:
//   reduce: sums[0:C] = sum g, sums[C:2C] = sum g*xhat2                          (BN2, over the output rows)
//           sums[2C:3C] = sum u = sum g, sums[3C:4C] = sum u*xhat0 = sum g*xhat0(pool(z0))   (BN0, over the full-resolution rows)
//           each [2C] half in iseg_bn_bwd_reduce's layout, so the SyncBN all-reduce carries the message unchanged.
//   apply:  dz2 = gamma2*rstd2*(g - sums0*inv_n2 - xhat2*sums1*inv_n2)   (training statistics; moving statistics: gamma2*rstd2*g)
//           dz0 = gamma0*rstd0*(u - sums2*inv_n0 - xhat0*sums3*inv_n0)   (BN0 shortcut) or dx = u (identity shortcut), on every full-res cell
//
// Streaming passes: a lane owns eight consecutive channels of an output row (16-byte bf16 / 2 x 16-byte fp32 accesses); a 256-lane workgroup
// tiles (row part, channel slab of <= 512 channels).  The reduce pass combines a workgroup's partial sums through LDS in row-lane order and
// writes them to the caller's workspace; a second launch sums the parts in a fixed order.  No floating-point atomics: the results are bitwise
// reproducible.  Storage fp32 or bf16, arithmetic fp32; C % 8 == 0.
#include "common.h"

namespace {

constexpr int RB_THREADS = 256;
constexpr int RB_SLAB_CHUNKS = 64;       // eight-channel chunks per workgroup slab (512 channels)
constexpr int RB_ROWS_PER_LANE = 8;      // output rows per lane and pass
constexpr int RB_MAX_PARTS = 4096;       // row parts of the reduce pass (bounds its workspace)
constexpr int RBF_PART_LANES = 64;       // the fixed-order part sum: 64 part lanes x 4 columns per workgroup

struct RbTile {
    int nchunks, tpc, rpi, slabs, parts;
    int64_t rows_per_part;
};

// Depends on the shape only, so the summation order (and the result bits) is a function of the shape.
RbTile rb_tile(int64_t P, int C) {
    RbTile t;
    t.nchunks = C / 8;
    t.tpc = t.nchunks < RB_SLAB_CHUNKS ? t.nchunks : RB_SLAB_CHUNKS;
    t.rpi = RB_THREADS / t.tpc;
    t.slabs = (t.nchunks + t.tpc - 1) / t.tpc;
    int64_t parts = ceil_div64(P, (int64_t)t.rpi * RB_ROWS_PER_LANE);
    if (parts > RB_MAX_PARTS) parts = RB_MAX_PARTS;
    if (parts < 1) parts = 1;
    t.rows_per_part = ceil_div64(P, parts);
    t.parts = (int)ceil_div64(P, t.rows_per_part);      // no empty part
    return t;
}

struct RbGeom {
    int H, W, Ho, Wo, C;
    int64_t P;      // N * Ho * Wo
};

// Lane geometry: channel chunk `cc` (global), row lane `tr`, output rows [r0, r1).
struct RbLane {
    int tc, tr, cc;
    bool active;
    int64_t r0, r1;
    __device__ RbLane(const RbTile& t, int64_t P) {
        tc = threadIdx.x % t.tpc;
        tr = threadIdx.x / t.tpc;
        cc = blockIdx.y * t.tpc + tc;
        active = tr < t.rpi && cc < t.nchunks;
        r0 = (int64_t)blockIdx.x * t.rows_per_part;
        r1 = r0 + t.rows_per_part < P ? r0 + t.rows_per_part : P;
    }
};

// The pooling window of output row r: element offsets (channel 0) of its valid full-resolution cells, and their count.
template <int S>
struct RbWindow {
    int64_t off[S * S];
    int cnt;
    __device__ __forceinline__ RbWindow(int64_t r, const RbGeom& g) {
        if (S == 1) {
            off[0] = r * g.C;
            cnt = 1;
        } else {
            const int64_t hw = (int64_t)g.Ho * g.Wo;
            const int64_t n = r / hw;
            const int rem = (int)(r - n * hw);
            const int oh = rem / g.Wo, ow = rem - (rem / g.Wo) * g.Wo;
            const int h0 = oh * S, w0 = ow * S;
            cnt = 0;
#pragma unroll
            for (int dy = 0; dy < S; ++dy)
#pragma unroll
                for (int dx = 0; dx < S; ++dx) {
                    const bool ok = h0 + dy < g.H && w0 + dx < g.W;
                    off[dy * S + dx] = ok ? ((n * g.H + h0 + dy) * g.W + w0 + dx) * g.C : -1;
                    cnt += ok ? 1 : 0;
                }
        }
    }
};

// mean over the window of the shortcut input (raw z0 or x), eight channels from c
template <class T, int S>
__device__ __forceinline__ void rb_pool(const T* __restrict__ sc, const RbWindow<S>& win, int c, float* v) {
    load8<T>(sc + win.off[0] + c, v);
    if (S > 1) {
#pragma unroll
        for (int k = 1; k < S * S; ++k) {
            if (win.off[k] < 0) continue;
            float w[8];
            load8<T>(sc + win.off[k] + c, w);
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] += w[u];
        }
        const float inv = 1.f / (float)win.cnt;
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] *= inv;
    }
}

template <class T, int S, bool BN0>
__global__ __launch_bounds__(RB_THREADS) void rb_fwd_kernel(const T* __restrict__ z2, const float* __restrict__ mean2,
                                                            const float* __restrict__ rstd2, const float* __restrict__ gamma2,
                                                            const float* __restrict__ beta2, const T* __restrict__ sc,
                                                            const float* __restrict__ mean0, const float* __restrict__ rstd0,
                                                            const float* __restrict__ gamma0, const float* __restrict__ beta0,
                                                            T* __restrict__ out, RbGeom g, RbTile t) {
    const RbLane L(t, g.P);
    if (!L.active) return;
    const int c = L.cc * 8;
    float k2[8], h2[8], k0[8], h0[8];
    {
        float m[8], rs[8], ga[8], b[8];
        load8<float>(mean2 + c, m);
        load8<float>(rstd2 + c, rs);
        load8<float>(gamma2 + c, ga);
        load8<float>(beta2 + c, b);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            k2[u] = rs[u] * ga[u];
            h2[u] = b[u] - m[u] * k2[u];
        }
        if (BN0) {
            load8<float>(mean0 + c, m);
            load8<float>(rstd0 + c, rs);
            load8<float>(gamma0 + c, ga);
            load8<float>(beta0 + c, b);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                k0[u] = rs[u] * ga[u];
                h0[u] = b[u] - m[u] * k0[u];
            }
        }
    }
    for (int64_t r = L.r0 + L.tr; r < L.r1; r += t.rpi) {
        const RbWindow<S> win(r, g);
        float z[8], s[8];
        load8<T>(z2 + r * g.C + c, z);
        rb_pool<T, S>(sc, win, c, s);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float sv = BN0 ? s[u] * k0[u] + h0[u] : s[u];
            const float v = z[u] * k2[u] + h2[u] + sv;
            z[u] = relu_f32(v);
        }
        store8<T>(out + r * g.C + c, z);
    }
}

// NQ quantities per (part, c): lanes put theirs in LDS [row lane][q][slab channel]; the first lanes sum them in row-lane order and write
// partials[(part * NQ + q) * C + c].
template <int NQ>
__device__ __forceinline__ void rb_flush(float (*acc)[8], const RbLane& L, const RbTile& t, int C, float* __restrict__ partials, float* lds) {
    const int sw = t.tpc * 8;
    if (L.tr < t.rpi) {      // lanes past the last chunk store zeros: every read cell is written
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int u = 0; u < 8; ++u) lds[((size_t)L.tr * NQ + q) * sw + L.tc * 8 + u] = L.active ? acc[q][u] : 0.f;
    }
    __syncthreads();
    const int cbase = blockIdx.y * sw;
    float* dst = partials + (int64_t)blockIdx.x * NQ * C;
    for (int i = threadIdx.x; i < NQ * sw; i += RB_THREADS) {
        const int q = i / sw, j = i % sw;
        if (cbase + j >= C) continue;
        float s = 0.f;
        for (int k = 0; k < t.rpi; ++k) s += lds[((size_t)k * NQ + q) * sw + j];
        dst[(int64_t)q * C + cbase + j] = s;
    }
}

// per (part, c): q0 = sum g, q1 = sum g*xhat2, and with a BN0 shortcut q2 = sum g*xhat0(pool(z0))
template <class T, int S, bool BN0>
__global__ __launch_bounds__(RB_THREADS) void rb_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                                   const T* __restrict__ z2, const float* __restrict__ mean2,
                                                                   const float* __restrict__ rstd2, const T* __restrict__ z0,
                                                                   const float* __restrict__ mean0, const float* __restrict__ rstd0,
                                                                   float* __restrict__ partials, RbGeom g, RbTile t) {
    constexpr int NQ = BN0 ? 3 : 2;
    __shared__ __attribute__((aligned(16))) float lds[NQ * RB_THREADS * 8];
    const RbLane L(t, g.P);
    float acc[NQ][8] = {};
    if (L.active) {
        const int c = L.cc * 8;
        float m2[8], rs2[8], m0[8], rs0[8];
        load8<float>(mean2 + c, m2);
        load8<float>(rstd2 + c, rs2);
        if (BN0) {
            load8<float>(mean0 + c, m0);
            load8<float>(rstd0 + c, rs0);
        }
        for (int64_t r = L.r0 + L.tr; r < L.r1; r += t.rpi) {
            float d[8], o[8], z[8], s[8];
            load8<T>(dout + r * g.C + c, d);
            load8<T>(out + r * g.C + c, o);
            load8<T>(z2 + r * g.C + c, z);
            if (BN0) {
                const RbWindow<S> win(r, g);
                rb_pool<T, S>(z0, win, c, s);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float gv = o[u] > 0.f ? d[u] : 0.f;
                acc[0][u] += gv;
                acc[1][u] += gv * ((z[u] - m2[u]) * rs2[u]);
                if (BN0) acc[NQ - 1][u] += gv * ((s[u] - m0[u]) * rs0[u]);
            }
        }
    }
    rb_flush<NQ>(acc, L, t, g.C, partials, lds);
}

// One lane per (q, c) column and part lane: the parts are summed in part order within a lane (p = lane, lane + 64, ...), the 64 part lanes
// by a fixed LDS tree.  Writes sums [2C] (identity) or [4C] (BN0; sum u = sum g fills [2C:3C]).
__global__ __launch_bounds__(RB_THREADS) void rb_bwd_sums_kernel(const float* __restrict__ partials, int parts, int NQ, int C,
                                                                 float* __restrict__ sums) {
    __shared__ float lds[RB_THREADS];
    constexpr int COLS = RB_THREADS / RBF_PART_LANES;
    const int col = blockIdx.x * COLS + threadIdx.x % COLS;
    const int pl = threadIdx.x / COLS;
    const int ncol = NQ * C;
    float s = 0.f;
    if (col < ncol) {
        const int64_t ps = (int64_t)ncol;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int p = pl;
        for (; p + 3 * RBF_PART_LANES < parts; p += 4 * RBF_PART_LANES) {
            a0 += partials[(int64_t)p * ps + col];
            a1 += partials[(int64_t)(p + RBF_PART_LANES) * ps + col];
            a2 += partials[(int64_t)(p + 2 * RBF_PART_LANES) * ps + col];
            a3 += partials[(int64_t)(p + 3 * RBF_PART_LANES) * ps + col];
        }
        for (; p < parts; p += RBF_PART_LANES) a0 += partials[(int64_t)p * ps + col];
        s = (a0 + a1) + (a2 + a3);
    }
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int half = RBF_PART_LANES / 2; half > 0; half >>= 1) {
        if (pl < half) lds[threadIdx.x] += lds[threadIdx.x + half * COLS];
        __syncthreads();
    }
    if (pl == 0 && col < ncol) {
        const float v = lds[threadIdx.x];
        const int q = col / C, c = col % C;
        if (q == 0) {
            sums[c] = v;
            if (NQ == 3) sums[2 * C + c] = v;
        } else if (q == 1) {
            sums[C + c] = v;
        } else {
            sums[3 * C + c] = v;
        }
    }
}

__device__ __forceinline__ void rb_book(float* __restrict__ dst, const float* v) {
    float a[8];
    load8<float>(dst, a);
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] += v[u];
    store8<float>(dst, a);
}

template <class T, int S, bool BN0>
__global__ __launch_bounds__(RB_THREADS) void rb_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ out,
                                                                  const T* __restrict__ z2, const float* __restrict__ mean2,
                                                                  const float* __restrict__ rstd2, const float* __restrict__ gamma2,
                                                                  const T* __restrict__ z0, const float* __restrict__ mean0,
                                                                  const float* __restrict__ rstd0, const float* __restrict__ gamma0,
                                                                  const float* __restrict__ sums, float inv_n2, float inv_n0, int train,
                                                                  T* __restrict__ dz2, T* __restrict__ dsc, float* __restrict__ dgamma2,
                                                                  float* __restrict__ dbeta2, float* __restrict__ dgamma0,
                                                                  float* __restrict__ dbeta0, RbGeom g, RbTile t) {
    const RbLane L(t, g.P);
    if (!L.active) return;
    const int C = g.C, c = L.cc * 8;
    float m2[8], rs2[8], k2[8], a2[8], b2[8];
    float m0[8], rs0[8], k0[8], a0[8], b0[8];
    {
        float ga[8], s0[8], s1[8];
        load8<float>(mean2 + c, m2);
        load8<float>(rstd2 + c, rs2);
        load8<float>(gamma2 + c, ga);
        load8<float>(sums + c, s0);
        load8<float>(sums + C + c, s1);
        if (blockIdx.x == 0 && L.tr == 0) {      // this replica's own sums: book the parameter gradients (one lane per chunk)
            if (dbeta2) rb_book(dbeta2 + c, s0);
            if (dgamma2) rb_book(dgamma2 + c, s1);
        }
        const float tr = train ? inv_n2 : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            k2[u] = ga[u] * rs2[u];
            a2[u] = s0[u] * tr;
            b2[u] = s1[u] * tr;
        }
        if (BN0) {
            load8<float>(mean0 + c, m0);
            load8<float>(rstd0 + c, rs0);
            load8<float>(gamma0 + c, ga);
            load8<float>(sums + 2 * C + c, s0);
            load8<float>(sums + 3 * C + c, s1);
            if (blockIdx.x == 0 && L.tr == 0) {
                if (dbeta0) rb_book(dbeta0 + c, s0);
                if (dgamma0) rb_book(dgamma0 + c, s1);
            }
            const float tr0 = train ? inv_n0 : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                k0[u] = ga[u] * rs0[u];
                a0[u] = s0[u] * tr0;
                b0[u] = s1[u] * tr0;
            }
        }
    }
    for (int64_t r = L.r0 + L.tr; r < L.r1; r += t.rpi) {
        const RbWindow<S> win(r, g);
        float d[8], o[8], z[8], gv[8];
        load8<T>(dout + r * C + c, d);
        load8<T>(out + r * C + c, o);
        load8<T>(z2 + r * C + c, z);
        const float inv_cnt = 1.f / (float)win.cnt;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            gv[u] = o[u] > 0.f ? d[u] : 0.f;
            z[u] = k2[u] * (gv[u] - a2[u] - (z[u] - m2[u]) * rs2[u] * b2[u]);
            gv[u] *= inv_cnt;      // u = g / count on each cell of the window
        }
        store8<T>(dz2 + r * C + c, z);
#pragma unroll
        for (int k = 0; k < S * S; ++k) {
            if (win.off[k] < 0) continue;
            float v[8];
            if (BN0) {
                load8<T>(z0 + win.off[k] + c, v);
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = k0[u] * (gv[u] - a0[u] - (v[u] - m0[u]) * rs0[u] * b0[u]);
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = gv[u];
            }
            store8<T>(dsc + win.off[k] + c, v);
        }
    }
}

bool rb_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool rb_shape_ok(int N, int H, int W, int C, int stride) {
    return N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && (stride == 1 || stride == 2);
}
RbGeom rb_geom(int N, int H, int W, int C, int stride) {
    RbGeom g;
    g.H = H;
    g.W = W;
    g.Ho = (H + stride - 1) / stride;
    g.Wo = (W + stride - 1) / stride;
    g.C = C;
    g.P = (int64_t)N * g.Ho * g.Wo;
    return g;
}
#define RB_UNSUPPORTED(what, N, H, W, C, s)                                                                                          \
    do {                                                                                                                             \
        iseg_set_error("%s: unsupported shape N=%d H=%d W=%d C=%d stride=%d (C %% 8 == 0, stride 1 or 2, 16-byte aligned tensors)", \
                       what, N, H, W, C, s);                                                                                         \
        return ISEG_ERR_UNSUPPORTED;                                                                                                 \
    } while (0)

// kernel<T, S, BN0> from the runtime (stride, bn0)
#define RB_KERNEL(KERNEL, T, stride, bn0) \
    (stride == 1 ? (bn0 ? KERNEL<T, 1, true> : KERNEL<T, 1, false>) : (bn0 ? KERNEL<T, 2, true> : KERNEL<T, 2, false>))

}  // namespace

extern "C" int iseg_resblock_tail_supported(int C, int stride, int dtype) {
    return C > 0 && C % 8 == 0 && (stride == 1 || stride == 2) && (dtype == ISEG_F32 || dtype == ISEG_BF16) ? 1 : 0;
}

extern "C" size_t iseg_resblock_tail_workspace_bytes(int N, int H, int W, int C, int stride, int bn0) {
    if (!rb_shape_ok(N, H, W, C, stride)) return 0;
    const RbGeom g = rb_geom(N, H, W, C, stride);
    const RbTile t = rb_tile(g.P, C);
    return (size_t)t.parts * (bn0 ? 3 : 2) * C * sizeof(float);
}

extern "C" int iseg_resblock_tail_fwd(const void* z2, const float* mean2, const float* rstd2, const float* gamma2, const float* beta2,
                                      const void* sc, const float* mean0, const float* rstd0, const float* gamma0, const float* beta0,
                                      void* out, int N, int H, int W, int C, int stride, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(z2 && mean2 && rstd2 && gamma2 && beta2 && sc && out, "iseg_resblock_tail_fwd: null pointer");
    const bool bn0 = mean0 != nullptr;
    ISEG_REQUIRE(!bn0 || (rstd0 && gamma0 && beta0), "iseg_resblock_tail_fwd: BN0 needs mean0, rstd0, gamma0 and beta0");
    if (!rb_shape_ok(N, H, W, C, stride) || !rb_aligned(z2) || !rb_aligned(sc) ||
        !rb_aligned(out) || !rb_aligned(mean2) || !rb_aligned(rstd2) || !rb_aligned(gamma2) || !rb_aligned(beta2) ||
        (bn0 && (!rb_aligned(mean0) || !rb_aligned(rstd0) || !rb_aligned(gamma0) || !rb_aligned(beta0))))
        RB_UNSUPPORTED("iseg_resblock_tail_fwd", N, H, W, C, stride);
    const RbGeom g = rb_geom(N, H, W, C, stride);
    const RbTile t = rb_tile(g.P, C);
    const dim3 grid(t.parts, t.slabs);
    return by_dtype(dtype, "iseg_resblock_tail_fwd", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(RB_KERNEL(rb_fwd_kernel, T, stride, bn0), grid, dim3(RB_THREADS), 0, stream, (const T*)z2, mean2, rstd2, gamma2, beta2,
                           (const T*)sc, mean0, rstd0, gamma0, beta0, (T*)out, g, t);
        return iseg_check_launch("iseg_resblock_tail_fwd");
    });
}

extern "C" int iseg_resblock_tail_bwd_reduce(const void* dout, const void* out, const void* z2, const float* mean2, const float* rstd2,
                                             const void* z0, const float* mean0, const float* rstd0, float* sums, int N, int H, int W, int C,
                                             int stride, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(dout && out && z2 && mean2 && rstd2 && sums && ws, "iseg_resblock_tail_bwd_reduce: null pointer");
    const bool bn0 = z0 != nullptr;
    ISEG_REQUIRE(!bn0 || (mean0 && rstd0), "iseg_resblock_tail_bwd_reduce: BN0 needs mean0 and rstd0");
    if (!rb_shape_ok(N, H, W, C, stride) || !rb_aligned(dout) || !rb_aligned(out) ||
        !rb_aligned(z2) || !rb_aligned(mean2) || !rb_aligned(rstd2) || (bn0 && (!rb_aligned(z0) || !rb_aligned(mean0) || !rb_aligned(rstd0))))
        RB_UNSUPPORTED("iseg_resblock_tail_bwd_reduce", N, H, W, C, stride);
    ISEG_NEED_WORKSPACE("iseg_resblock_tail_bwd_reduce", ws, ws_bytes, iseg_resblock_tail_workspace_bytes(N, H, W, C, stride, bn0));
    const RbGeom g = rb_geom(N, H, W, C, stride);
    const RbTile t = rb_tile(g.P, C);
    float* partials = (float*)ws;
    const int rc = by_dtype(dtype, "iseg_resblock_tail_bwd_reduce", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(RB_KERNEL(rb_bwd_reduce_kernel, T, stride, bn0), dim3(t.parts, t.slabs), dim3(RB_THREADS), 0, stream, (const T*)dout,
                           (const T*)out, (const T*)z2, mean2, rstd2, (const T*)z0, mean0, rstd0, partials, g, t);
    });
    if (rc != ISEG_OK) return rc;
    const int NQ = bn0 ? 3 : 2;
    const int cols_per_block = RB_THREADS / RBF_PART_LANES;
    hipLaunchKernelGGL(rb_bwd_sums_kernel, dim3((unsigned)ceil_div64((int64_t)NQ * C, cols_per_block)), dim3(RB_THREADS), 0, stream, partials,
                       t.parts, NQ, C, sums);
    return iseg_check_launch("iseg_resblock_tail_bwd_reduce");
}

extern "C" int iseg_resblock_tail_bwd_apply(const void* dout, const void* out, const void* z2, const float* mean2, const float* rstd2,
                                            const float* gamma2, const void* z0, const float* mean0, const float* rstd0, const float* gamma0,
                                            const float* sums, float inv_n2, float inv_n0, int train, void* dz2, void* dsc, float* dgamma2,
                                            float* dbeta2, float* dgamma0, float* dbeta0, int N, int H, int W, int C, int stride, int dtype,
                                            hipStream_t stream) {
    ISEG_REQUIRE(dout && out && z2 && mean2 && rstd2 && gamma2 && sums && dz2 && dsc, "iseg_resblock_tail_bwd_apply: null pointer");
    const bool bn0 = z0 != nullptr;
    ISEG_REQUIRE(!bn0 || (mean0 && rstd0 && gamma0), "iseg_resblock_tail_bwd_apply: BN0 needs mean0, rstd0 and gamma0");
    if (!rb_shape_ok(N, H, W, C, stride) || !rb_aligned(dout) || !rb_aligned(out) ||
        !rb_aligned(z2) || !rb_aligned(dz2) || !rb_aligned(dsc) || !rb_aligned(mean2) || !rb_aligned(rstd2) || !rb_aligned(gamma2) ||
        !rb_aligned(sums) || (bn0 && (!rb_aligned(z0) || !rb_aligned(mean0) || !rb_aligned(rstd0) || !rb_aligned(gamma0))) ||
        (dgamma2 && !rb_aligned(dgamma2)) || (dbeta2 && !rb_aligned(dbeta2)) || (dgamma0 && !rb_aligned(dgamma0)) ||
        (dbeta0 && !rb_aligned(dbeta0)))
        RB_UNSUPPORTED("iseg_resblock_tail_bwd_apply", N, H, W, C, stride);
    const RbGeom g = rb_geom(N, H, W, C, stride);
    const RbTile t = rb_tile(g.P, C);
    return by_dtype(dtype, "iseg_resblock_tail_bwd_apply", [&](auto st) {
        using T = decltype(st);
        hipLaunchKernelGGL(RB_KERNEL(rb_bwd_apply_kernel, T, stride, bn0), dim3(t.parts, t.slabs), dim3(RB_THREADS), 0, stream, (const T*)dout,
                           (const T*)out, (const T*)z2, mean2, rstd2, gamma2, (const T*)z0, mean0, rstd0, gamma0, sums, inv_n2, inv_n0, train, (T*)dz2,
                           (T*)dsc, dgamma2, dbeta2, bn0 ? dgamma0 : nullptr, bn0 ? dbeta0 : nullptr, g, t);
        return iseg_check_launch("iseg_resblock_tail_bwd_apply");
    });
}
