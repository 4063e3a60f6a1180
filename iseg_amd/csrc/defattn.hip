// Deformable multi-head self-attention core of the reference (layers/deformable_multihead_self_attention.py:89-244), one kernel each way:
//
//   value [N, H, W, heads * Ch], offset logits [N, H, W, heads * P * 2] read as [heads, P, (y, x)] (:196-199), attention logits [N, H, W, heads * P]
//   t  = tanh(offset logits);  dy = t_y * (H / offset_range_factor),  dx = t_x * (W / offset_range_factor)                      (:203-207)
//   a  = softmax over the P points of a head                                                                                    (:210-214)
//   y  = clip(h + dy, 0, H - 1),  x = clip(w + dx, 0, W - 1)                                                                    (:225-230)
//   y0 = floor(y), y1 = y0 + 1 (x likewise), indices clipped to the image; wy1 = y - y0, wy0 = 1 - wy1 from the UNCLIPPED y0    (:124-137)
//   sample_p = wy0 wx0 v[y0,x0] + wy0 wx1 v[y0,x1] + wy1 wx0 v[y1,x0] + wy1 wx1 v[y1,x1]   over the head's Ch channels         (:154-169)
//   out[n,h,w,head,:] = sum_p a_p sample_p                                                                                      (:236-240)
//
// tanh, softmax, coordinates and bilinear weights are fp32 whatever the storage dtype (the reference computes them in the compute dtype; same
// decision as dcnv3.hip).  The reference's scrub of the softmax weights (:215) is an identity on finite values and is not reproduced; the scrubs of
// query / value / out (:182-183, :242) are the layer's (iseg_amd/layers/deformable_multihead_self_attention.py).
//
// Gradients: clip passes where the unclipped coordinate lies in [0, H - 1] (bounds included, as tf.clip_by_value), floor has none.
//   dvalue[corner k of p] += dout a_p w_k           int64 2^-40 fixed-point atomics into a zeroed workspace + unfix pass (dcn_fixed.h): order-free
//   g_p   = <dout, sample_p>                        dattn_p = a_p (g_p - sum_q a_q g_q)
//   gy_p  = <dout, d sample_p / dy>                 doffset_y = a_p gy_p [0 <= h + dy <= H - 1] (H / orf) (1 - t_y^2), x likewise
// The channel sums are lane-group sums (DPP, fixed order); nothing but the three operands is read back from the forward.
#include "common.h"
#include "dcn_fixed.h"
#include "iseg_hip.h"
#include <math.h>

namespace {

constexpr int DA_PMAX = 16;      // sampling points per head the kernels keep in registers

struct DaGeom {
    int N, H, W, heads, P, Ch;
    float sy, sx;      // H / offset_range_factor, W / offset_range_factor
};

struct DaTap {
    int y0, y1, x0, x1;               // clipped corner indices
    float wy0, wy1, wx0, wx1;         // from the unclipped floor
    float ky, kx;                     // d coordinate / d offset logit: clip mask * scale * (1 - tanh^2)
};

__device__ __forceinline__ DaTap da_tap(const DaGeom& g, int h, int w, float oy, float ox) {
    const float ty = tanhf(oy), tx = tanhf(ox);
    const float yu = (float)h + ty * g.sy, xu = (float)w + tx * g.sx;
    const float hy = (float)(g.H - 1), hx = (float)(g.W - 1);
    const float y = fminf(fmaxf(yu, 0.f), hy), x = fminf(fmaxf(xu, 0.f), hx);      // (a NaN coordinate clips to 0: every address stays inside the image)
    const float fy = floorf(y), fx = floorf(x);
    DaTap t;
    t.wy1 = y - fy;
    t.wx1 = x - fx;
    t.wy0 = 1.f - t.wy1;
    t.wx0 = 1.f - t.wx1;
    const int iy = (int)fy, ix = (int)fx;
    t.y0 = min(max(iy, 0), g.H - 1);
    t.y1 = min(max(iy + 1, 0), g.H - 1);
    t.x0 = min(max(ix, 0), g.W - 1);
    t.x1 = min(max(ix + 1, 0), g.W - 1);
    t.ky = (yu >= 0.f && yu <= hy) ? g.sy * (1.f - ty * ty) : 0.f;
    t.kx = (xu >= 0.f && xu <= hx) ? g.sx * (1.f - tx * tx) : 0.f;
    return t;
}

// logits of one (pixel, head) -> offsets as stored and softmax weights; entries p >= P repeat point P - 1 (loads stay in bounds, results unused)
template <class T, int PMAX>
__device__ __forceinline__ void da_points(const T* __restrict__ op, const T* __restrict__ ap, int P, float* oy, float* ox, float* a) {
    float m = -INFINITY;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) {
        const int pp = p < P ? p : P - 1;
        oy[p] = to_f32(op[2 * pp]);
        ox[p] = to_f32(op[2 * pp + 1]);
        a[p] = to_f32(ap[pp]);
        m = fmaxf(m, a[p]);
    }
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) {
        a[p] = expf(a[p] - m);
        if (p < P) s += a[p];
    }
    const float r = 1.f / s;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) a[p] *= r;
}

// Forward, Ch % 8 == 0: a lane owns 8 consecutive channels of one (pixel, head); the Ch / 8 lanes of a head are neighbours, so a corner read is one
// contiguous run of Ch elements.  Like dcnv3_fwd_pipe_kernel the kernel is a chain of dependent round trips (logits -> tap -> four corner rows), so
// all logits are loaded up front and the corner rows of point p + 1 are requested before point p is accumulated.
template <class T, int PMAX>
__global__ __launch_bounds__(256) void defattn_fwd_vec_kernel(const T* __restrict__ value, const T* __restrict__ off, const T* __restrict__ attn,
                                                              T* __restrict__ out, DaGeom g) {
    constexpr int RAW = 8 * (int)sizeof(T) / 16;
    const int P = g.P, CV = g.Ch / 8, HC = g.heads * CV;
    const int64_t C = (int64_t)g.heads * g.Ch;
    const int64_t total = (int64_t)g.N * g.H * g.W * HC;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int hc = (int)(i % HC);
        const int64_t pix = i / HC;
        const int head = hc / CV;
        const int w = (int)(pix % g.W), h = (int)((pix / g.W) % g.H);
        const int64_t n = pix / ((int64_t)g.W * g.H);
        float oy[PMAX], ox[PMAX], a[PMAX];
        da_points<T, PMAX>(off + (pix * g.heads + head) * P * 2, attn + (pix * g.heads + head) * P, P, oy, ox, a);
        const T* const vb = value + n * g.H * g.W * C + hc * 8;      // this lane's channels of pixel (0, 0) of image n
        uint4 nxt[4][RAW];
        DaTap ntp{};
        auto request = [&](int p) {
            ntp = da_tap(g, h, w, oy[p], ox[p]);
            const int ys[4] = {ntp.y0, ntp.y0, ntp.y1, ntp.y1};
            const int xs[4] = {ntp.x0, ntp.x1, ntp.x0, ntp.x1};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4* q = reinterpret_cast<const uint4*>(vb + ((int64_t)ys[k] * g.W + xs[k]) * C);
#pragma unroll
                for (int r = 0; r < RAW; ++r) nxt[k][r] = q[r];
            }
        };
        request(0);
        float acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = 0.f;
#pragma unroll
        for (int p = 0; p < PMAX; ++p) {
            if (p >= P) continue;
            const DaTap tp = ntp;
            float v[4][8];
#pragma unroll
            for (int k = 0; k < 4; ++k) dcn_unpack_row<T, 8>(nxt[k], v[k]);
            if (p + 1 < P) request(p + 1);
            const float wgt[4] = {tp.wy0 * tp.wx0, tp.wy0 * tp.wx1, tp.wy1 * tp.wx0, tp.wy1 * tp.wx1};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) s = fmaf(wgt[k], v[k][u], s);
                acc[u] = fmaf(a[p], s, acc[u]);
            }
        }
        store8<T>(out + i * 8, acc);
    }
}

// Forward, any Ch: a lane owns one channel of one (pixel, head)
template <class T>
__global__ __launch_bounds__(256) void defattn_fwd_kernel(const T* __restrict__ value, const T* __restrict__ off, const T* __restrict__ attn,
                                                          T* __restrict__ out, DaGeom g) {
    const int P = g.P;
    const int64_t C = (int64_t)g.heads * g.Ch;
    const int64_t total = (int64_t)g.N * g.H * g.W * C;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t pix = i / C;
        const int head = c / g.Ch;
        const int w = (int)(pix % g.W), h = (int)((pix / g.W) % g.H);
        const int64_t n = pix / ((int64_t)g.W * g.H);
        const T* const op = off + (pix * g.heads + head) * P * 2;
        const T* const ap = attn + (pix * g.heads + head) * P;
        float m = -INFINITY, s = 0.f;
        for (int p = 0; p < P; ++p) m = fmaxf(m, to_f32(ap[p]));
        for (int p = 0; p < P; ++p) s += expf(to_f32(ap[p]) - m);
        const float r = 1.f / s;
        const T* const vb = value + n * g.H * g.W * C + c;
        float acc = 0.f;
        for (int p = 0; p < P; ++p) {
            const DaTap tp = da_tap(g, h, w, to_f32(op[2 * p]), to_f32(op[2 * p + 1]));
            const float v00 = to_f32(vb[((int64_t)tp.y0 * g.W + tp.x0) * C]), v01 = to_f32(vb[((int64_t)tp.y0 * g.W + tp.x1) * C]);
            const float v10 = to_f32(vb[((int64_t)tp.y1 * g.W + tp.x0) * C]), v11 = to_f32(vb[((int64_t)tp.y1 * g.W + tp.x1) * C]);
            float sm = tp.wy0 * tp.wx0 * v00;
            sm = fmaf(tp.wy0 * tp.wx1, v01, sm);
            sm = fmaf(tp.wy1 * tp.wx0, v10, sm);
            sm = fmaf(tp.wy1 * tp.wx1, v11, sm);
            acc = fmaf(expf(to_f32(ap[p]) - m) * r, sm, acc);
        }
        out[i] = from_f32<T>(acc);
    }
}

// Backward: LC lanes (a power of two) share one (pixel, head); lane c owns channels c, c + LC, ... of the head, so every corner load and every
// atomic of a wave-instruction is one contiguous run of min(Ch, LC) elements per item -- at the head shapes (Ch 64 / 128, LC 64) a whole wavefront
// adds into 512 contiguous bytes.  The channel reductions behind the logit gradients are log2(LC) DPP steps in a fixed order; the tap geometry and
// the softmax are recomputed by each lane.  dvalue: dcn_to_fixed atomics into `acc` (zeroed by the caller), converted by dcn_unfix_kernel.
template <class T, int LC, int PMAX>
__global__ __launch_bounds__(256) void defattn_bwd_kernel(const T* __restrict__ value, const T* __restrict__ off, const T* __restrict__ attn,
                                                          const T* __restrict__ dout, unsigned long long* __restrict__ acc, T* __restrict__ doff,
                                                          T* __restrict__ dattn, int* __restrict__ flag, DaGeom g) {
    const int P = g.P;
    const int64_t C = (int64_t)g.heads * g.Ch;
    const int64_t total = (int64_t)g.N * g.H * g.W * g.heads;      // (pixel, head) items
    const int lc = threadIdx.x % LC;
    constexpr int IPB = 256 / LC;
    bool bad = false;      // a non-finite contribution: the fixed-point conversion would saturate it to finite garbage (see dcn_unfix_kernel)
    for (int64_t i = blockIdx.x * (int64_t)IPB + threadIdx.x / LC; i < total; i += (int64_t)gridDim.x * IPB) {
        const int head = (int)(i % g.heads);
        const int64_t pix = i / g.heads;
        const int w = (int)(pix % g.W), h = (int)((pix / g.W) % g.H);
        const int64_t n = pix / ((int64_t)g.W * g.H);
        float oy[PMAX], ox[PMAX], a[PMAX], gp[PMAX];
        da_points<T, PMAX>(off + i * P * 2, attn + i * P, P, oy, ox, a);
        const int64_t vb = n * g.H * g.W * C + (int64_t)head * g.Ch;      // the head's channels of pixel (0, 0) of image n
        const T* const dp = dout + i * g.Ch;
        float S = 0.f;
#pragma unroll
        for (int p = 0; p < PMAX; ++p) {
            gp[p] = 0.f;
            if (p >= P) continue;
            const DaTap tp = da_tap(g, h, w, oy[p], ox[p]);
            const int64_t e00 = vb + ((int64_t)tp.y0 * g.W + tp.x0) * C, e01 = vb + ((int64_t)tp.y0 * g.W + tp.x1) * C;
            const int64_t e10 = vb + ((int64_t)tp.y1 * g.W + tp.x0) * C, e11 = vb + ((int64_t)tp.y1 * g.W + tp.x1) * C;
            const float w00 = tp.wy0 * tp.wx0, w01 = tp.wy0 * tp.wx1, w10 = tp.wy1 * tp.wx0, w11 = tp.wy1 * tp.wx1;
            float gm = 0.f, gy = 0.f, gx = 0.f;
            for (int c = lc; c < g.Ch; c += LC) {
                const float d = to_f32(dp[c]);
                const float v00 = to_f32(value[e00 + c]), v01 = to_f32(value[e01 + c]);
                const float v10 = to_f32(value[e10 + c]), v11 = to_f32(value[e11 + c]);
                const float da = d * a[p] * DCN_FIX;
                const float c00 = da * w00, c01 = da * w01, c10 = da * w10, c11 = da * w11;
                bad |= !(fabsf(c00) < 3.0e38f) | !(fabsf(c01) < 3.0e38f) | !(fabsf(c10) < 3.0e38f) | !(fabsf(c11) < 3.0e38f);
                atomicAdd(acc + e00 + c, dcn_to_fixed(c00));
                atomicAdd(acc + e01 + c, dcn_to_fixed(c01));
                atomicAdd(acc + e10 + c, dcn_to_fixed(c10));
                atomicAdd(acc + e11 + c, dcn_to_fixed(c11));
                float sm = w00 * v00;
                sm = fmaf(w01, v01, sm);
                sm = fmaf(w10, v10, sm);
                sm = fmaf(w11, v11, sm);
                gm = fmaf(d, sm, gm);
                gy = fmaf(d, fmaf(tp.wx0, v10 - v00, tp.wx1 * (v11 - v01)), gy);
                gx = fmaf(d, fmaf(tp.wy0, v01 - v00, tp.wy1 * (v11 - v10)), gx);
            }
            gm = group_sum(gm, LC);
            gy = group_sum(gy, LC);
            gx = group_sum(gx, LC);
            gp[p] = gm;
            S = fmaf(a[p], gm, S);
            if (lc == 0) {
                doff[(i * P + p) * 2] = from_f32<T>(a[p] * gy * tp.ky);
                doff[(i * P + p) * 2 + 1] = from_f32<T>(a[p] * gx * tp.kx);
            }
        }
        if (lc == 0) {
#pragma unroll
            for (int p = 0; p < PMAX; ++p)
                if (p < P) dattn[i * P + p] = from_f32<T>(a[p] * (gp[p] - S));
        }
    }
    if (bad) atomicOr(flag, 2);      // (rare; integer OR: order-free)
}

static int da_geom(DaGeom* g, int N, int H, int W, int heads, int P, int Ch, float orf, const char* who) {
    ISEG_REQUIRE(N > 0 && H > 0 && W > 0 && heads > 0 && Ch > 0 && orf > 0.f, "%s: bad geometry", who);
    if (P < 1 || P > DA_PMAX) {
        iseg_set_error("%s: %d sampling points per head (1..%d are built)", who, P, DA_PMAX);
        return ISEG_ERR_UNSUPPORTED;
    }
    ISEG_REQUIRE((int64_t)N * H * W * heads * (Ch > 2 * P ? Ch : 2 * P) < (1ll << 40), "%s: tensor too large", who);
    g->N = N; g->H = H; g->W = W; g->heads = heads; g->P = P; g->Ch = Ch;
    g->sy = (float)((double)H / (double)orf);
    g->sx = (float)((double)W / (double)orf);
    return ISEG_OK;
}

// nel int64 accumulators (rounded up to 16 bytes) + a 16-byte slot whose first word is the non-finite flag
static size_t da_ws_bytes(int64_t nel) { return ((size_t)nel * sizeof(unsigned long long) + 15) / 16 * 16 + 16; }

}  // namespace

extern "C" int iseg_defattn_fwd(const void* value, const void* offset_logits, const void* attn_logits, void* out, int N, int H, int W, int heads,
                                int P, int Ch, float offset_range_factor, int dtype, hipStream_t stream) {
    ISEG_REQUIRE(value && offset_logits && attn_logits && out, "iseg_defattn_fwd: null pointer");
    DaGeom g;
    const int rc = da_geom(&g, N, H, W, heads, P, Ch, offset_range_factor, "iseg_defattn_fwd");
    if (rc != ISEG_OK) return rc;
    const bool v8 = Ch % 8 == 0 && (uintptr_t)value % 16 == 0 && (uintptr_t)out % 16 == 0;
    const int64_t lanes = (int64_t)N * H * W * heads * (v8 ? Ch / 8 : Ch);
    return by_dtype(dtype, "iseg_defattn_fwd", [&](auto t) {
        using T = decltype(t);
        const auto kernel = v8 ? (P <= 4 ? defattn_fwd_vec_kernel<T, 4> : defattn_fwd_vec_kernel<T, DA_PMAX>) : defattn_fwd_kernel<T>;
        hipLaunchKernelGGL(kernel, dim3(lane_blocks(lanes)), dim3(256), 0, stream, (const T*)value, (const T*)offset_logits, (const T*)attn_logits,
                           (T*)out, g);
        return iseg_check_launch("iseg_defattn_fwd");
    });
}

extern "C" size_t iseg_defattn_bwd_workspace_bytes(int N, int H, int W, int heads, int Ch) {
    if (N <= 0 || H <= 0 || W <= 0 || heads <= 0 || Ch <= 0) return 0;
    return da_ws_bytes((int64_t)N * H * W * heads * Ch);
}

extern "C" int iseg_defattn_bwd(const void* value, const void* offset_logits, const void* attn_logits, const void* dout, void* dvalue,
                                void* doffset_logits, void* dattn_logits, int N, int H, int W, int heads, int P, int Ch, float offset_range_factor,
                                int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(value && offset_logits && attn_logits && dout && dvalue && doffset_logits && dattn_logits, "iseg_defattn_bwd: null pointer");
    ISEG_REQUIRE(dtype == ISEG_BF16 || dtype == ISEG_F32, "iseg_defattn_bwd: dtype %d", dtype);      // (before the first launch)
    DaGeom g;
    const int rc = da_geom(&g, N, H, W, heads, P, Ch, offset_range_factor, "iseg_defattn_bwd");
    if (rc != ISEG_OK) return rc;
    const int64_t nel = (int64_t)N * H * W * heads * Ch;
    const size_t need = da_ws_bytes(nel);
    ISEG_NEED_WORKSPACE("iseg_defattn_bwd", ws, ws_bytes, need);
    ISEG_REQUIRE_WORKSPACE((uintptr_t)ws % 16 == 0, "iseg_defattn_bwd: the workspace must be 16-byte aligned");
    const int64_t n16 = (int64_t)need / 16;      // (accumulators and the flag slot are zeroed by one launch)
    hipLaunchKernelGGL(dcn_zero_kernel, dim3(lane_blocks(n16)), dim3(256), 0, stream, (uint4*)ws, n16);
    unsigned long long* const acc = (unsigned long long*)ws;
    int* const flag = (int*)((char*)ws + need - 16);
    const int64_t items = (int64_t)N * H * W * heads;
    return by_dtype(dtype, "iseg_defattn_bwd", [&](auto t) {
        using T = decltype(t);
        auto launch = [&](auto kernel4, auto kernel, int lc) {
            hipLaunchKernelGGL((P <= 4 ? kernel4 : kernel), dim3(lane_blocks(items * lc)), dim3(256), 0, stream, (const T*)value, (const T*)offset_logits,
                               (const T*)attn_logits, (const T*)dout, acc, (T*)doffset_logits, (T*)dattn_logits, flag, g);
        };
        if (Ch <= 4) launch(defattn_bwd_kernel<T, 4, 4>, defattn_bwd_kernel<T, 4, DA_PMAX>, 4);
        else if (Ch <= 16) launch(defattn_bwd_kernel<T, 16, 4>, defattn_bwd_kernel<T, 16, DA_PMAX>, 16);
        else launch(defattn_bwd_kernel<T, 64, 4>, defattn_bwd_kernel<T, 64, DA_PMAX>, 64);
        hipLaunchKernelGGL(dcn_unfix_kernel<T>, dim3(lane_blocks(nel)), dim3(256), 0, stream, acc, (T*)dvalue, nel, (const int*)flag);
        return iseg_check_launch("iseg_defattn_bwd");
    });
}
