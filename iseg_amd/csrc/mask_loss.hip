// MaskLoss (losses/mask_loss.py:10-201 on losses/seg_loss_base.py:12-95): per-class sigmoid (focal) loss + per-image dice loss + softmax
// cross-entropy with the ignore label carried as a Keras loss mask, fp32, loss AND gradient in two streaming passes over the logits.
//
//   valid = y != ignore ; (ignore == 0 -> y -= 1) ; t = onehot(y) is the zero row for every y outside [0, C)
//   sigmoid term   k_s * mean_c f(z_c, t_c):  bce = max(z,0) - z t + log1p(exp(-|z|)) ;  f = bce, or (1 - p_t)^2 * bce * w  (gamma = 2,
//                  w = t alpha + (1 - t)(1 - alpha) under class balancing, alpha = 0.25: the Keras defaults MaskLoss leaves in place)
//   dice term      k_d * (1 - I_b / D_b),  I_b = 2 sum valid s t + 1e-7,  D_b = sum valid s + sum valid t + 1e-7   (per image b)
//   CE term        k_c * (lse(z) - z_y), or Keras' categorical_focal_crossentropy (alpha 0.25, gamma 2) ; zero where t is the zero row
//   L = sum_p valid_p l_p / (V + 1e-7),  V = sum valid      (Keras' masked sum_over_batch_size reduction: a mean over VALID pixels)
//
// Everything but I_b, D_b, V is pixel-local:
//   pass 1    streams the logits, leaves per-tile partial sums (a tile never crosses an image) and log-sum-exp per pixel;
//   finalize  one workgroup adds the partials in a fixed order -> V, dice_b, the dice gradient coefficients per image, L (all on the device);
//   pass 2    streams the logits again and writes
//             dL/dz = g_p [k_s dsig + k_c dce] + W_b k_d valid s (1 - s) (I_b / D_b^2 - 2 t / D_b),
//             g_p = grad_scale * valid / (V + 1e-7), W_b = grad_scale * V_b / (V + 1e-7)                    (scalar route), or
//             g_p = grad_scale * valid * grad_px[p], W_b = grad_scale * sum_p grad_px[p] valid_p            (per-pixel upstream gradient).
// No floating-point atomics: every sum is a fixed-order tree, so loss and gradient are bit-reproducible.
// Tile shape as csrc/loss.hip: PIX pixels x C logits staged through LDS with coalesced 16-B lanes, one lane per pixel (row stride C words,
// conflict-free for odd C), the gradient row goes back into the same LDS slab and is streamed out coalesced.
// The t = 0 branch is evaluated for every class and the one class with t = 1 is corrected afterwards (no per-element select).
#include "common.h"
#include "iseg_hip.h"

namespace {

constexpr int NPART = 8;             // floats per tile record: local, s*t, s, t, valid, grad_px*valid
constexpr float F_ALPHA = 0.25f;     // keras binary_focal_crossentropy / categorical_focal_crossentropy defaults (gamma = 2 is written as squares)
constexpr float K_EPS = 1e-7f;       // keras.backend.epsilon()

static inline int mask_loss_pix(int C) {
    int pix = (48 * 1024) / (4 * C);
    pix = (pix / 64) * 64;
    if (pix > 256) pix = 256;
    if (pix < 64) pix = 64;
    return pix;
}

struct Sig {
    float s, oms, bce0;      // sigmoid(z), 1 - sigmoid(z), softplus(z) = the t = 0 binary cross-entropy
};

template <bool WANT_BCE> __device__ __forceinline__ Sig sigmoid_parts(float z) {
    Sig r;
    const float e = __expf(-fabsf(z));
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float big = inv, small = e * inv;
    r.s = z >= 0.f ? big : small;
    r.oms = z >= 0.f ? small : big;
    r.bce0 = WANT_BCE ? fmaxf(z, 0.f) + __logf(1.f + e) : 0.f;
    return r;
}

__device__ __forceinline__ void stage_in(float* tile, const float* src, int64_t nel, bool vec) {
    if (vec) {
        for (int i = threadIdx.x; i < nel / 4; i += 256) reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < nel; i += 256) tile[i] = src[i];
    }
}

// SIG: 0 off, 1 plain binary cross-entropy, 2 focal ; CE: 0 off, 1 plain, 2 focal
template <int SIG, bool DICE, int CE>
__global__ __launch_bounds__(256) void mask_loss_pass1_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int64_t HW,
                                                              int C, int ignore, int tpi, int pix, float ks_c, float kc, float w0, float w1,
                                                              const float* __restrict__ grad_px, float* __restrict__ local_px,
                                                              float* __restrict__ lse_px, float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [pix][C]
    __shared__ float wsum[4][NPART];
    const int64_t tl = blockIdx.x;
    const int64_t b = tl / tpi;
    const int64_t q0 = (tl - b * tpi) * pix;
    const int npx = (int)((HW - q0 < pix) ? (HW - q0) : pix);
    const int64_t p0 = b * HW + q0;
    const int64_t nel = (int64_t)npx * C;
    stage_in(tile, logits + p0 * C, nel, ((p0 * C) % 4 == 0) && (nel % 4 == 0));
    __syncthreads();
    float loc = 0.f, a_st = 0.f, a_s = 0.f, a_t = 0.f, a_v = 0.f, a_g = 0.f;
    if ((int)threadIdx.x < npx) {
        const float* z = tile + threadIdx.x * C;
        int y = labels[p0 + threadIdx.x];
        const bool keep = y != ignore;
        if (ignore == 0) y -= 1;
        const bool in_range = y >= 0 && y < C;
        if (keep) {      // the reference evaluates ignored pixels too and masks them afterwards: same result
            const float zy = in_range ? z[y] : 0.f;
            float sig_sum = 0.f, s_sum = 0.f, mx = z[0];
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const float zc = z[c];
                if (CE) mx = fmaxf(mx, zc);
                if (SIG || DICE) {
                    const Sig q = sigmoid_parts<SIG != 0>(zc);
                    s_sum += q.s;
                    if (SIG == 1) sig_sum += q.bce0;
                    if (SIG == 2) sig_sum += (q.s * q.s) * q.bce0;
                }
            }
            if (SIG == 2) sig_sum *= w0;
            float s_y = 0.f;
            if ((SIG || DICE) && in_range) {
                const Sig q = sigmoid_parts<SIG != 0>(zy);
                s_y = q.s;
                if (SIG == 1) sig_sum -= zy;      // bce(t = 1) = bce(t = 0) - z
                if (SIG == 2) sig_sum += w1 * (q.oms * q.oms) * (q.bce0 - zy) - w0 * (q.s * q.s) * q.bce0;
            }
            float v = SIG ? ks_c * sig_sum : 0.f;
            if (CE) {
                float se = 0.f;
#pragma unroll 4
                for (int c = 0; c < C; ++c) se += __expf(z[c] - mx);
                const float lse = mx + __logf(se);
                if (lse_px) lse_px[p0 + threadIdx.x] = lse;
                if (in_range) {
                    if (CE == 1) {
                        v += kc * (lse - zy);
                    } else {
                        // keras CategoricalFocalCrossentropy(from_logits): p = clip(softmax_y, 1e-7, 1 - 1e-7), alpha (1 - p)^2 (-log p)
                        const float pc = clip_f32(__expf(zy - lse), 1e-7f, 1.f - 1e-7f);      // (NaN stays NaN and meets the scrub below)
                        const float om = 1.f - pc;
                        v += kc * F_ALPHA * (om * om) * (-__logf(pc));
                    }
                }
            }
            if (!(v == v)) v = 0.f;      // replace_nan_or_inf(., 0) of the reference, for NaN (finite logits never get here)
            loc = v;
            a_v = 1.f;
            a_s = s_sum;
            a_st = s_y;
            a_t = in_range ? 1.f : 0.f;
            if (grad_px) a_g = grad_px[p0 + threadIdx.x];
        }
        if (local_px) local_px[p0 + threadIdx.x] = loc;
    }
    float part[6] = {loc, a_st, a_s, a_t, a_v, a_g};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float s = wave_sum(part[k]);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 6) partials[tl * NPART + threadIdx.x] = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
}

// One workgroup of 16 wavefronts.  A wavefront adds the tile records of an image (lanes stride over the tiles, then a butterfly: the same
// order every run); thread 0 then walks the images in order.  img[b] = {cA, cB, k_d dice_b, I, D, V_b, ., .}, glob = {pixel factor, V}.
__global__ __launch_bounds__(1024) void mask_loss_finalize_kernel(const float* __restrict__ partials, int B, int tpi, float kd, int use_dice,
                                                                  int has_grad_px, float grad_scale, float loss_scale,
                                                                  float* __restrict__ img, float* __restrict__ glob, float* __restrict__ loss_out) {
    __shared__ float s_V;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int b = wid; b < B; b += 16) {
        float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = lane; t < tpi; t += 64) {
            const float* r = partials + ((int64_t)b * tpi + t) * NPART;
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] += r[k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] = wave_sum(acc[k]);
        if (lane == 0) {
            float* o = img + (int64_t)b * NPART;
            o[3] = 2.f * acc[1] + K_EPS;             // I_b
            o[4] = acc[2] + acc[3] + K_EPS;          // D_b
            o[5] = acc[4];                           // V_b
            o[6] = acc[0];                           // sum of the masked pixel-local terms
            o[7] = acc[5];                           // sum grad_px * valid
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float V = 0.f;
        for (int b = 0; b < B; ++b) V += img[(int64_t)b * NPART + 5];
        float num = 0.f;
        for (int b = 0; b < B; ++b) {
            const float* o = img + (int64_t)b * NPART;
            const float dice = use_dice ? kd * (1.f - o[3] / o[4]) : 0.f;      // D_b >= 1e-7: divide_no_nan never takes its zero branch
            num += o[6] + dice * o[5];
        }
        s_V = V;
        glob[0] = has_grad_px ? grad_scale : grad_scale / (V + K_EPS);
        glob[1] = V;
        if (loss_out) loss_out[0] = loss_scale * num / (V + K_EPS);
    }
    __syncthreads();
    const float V = s_V;
    for (int b = threadIdx.x; b < B; b += 1024) {
        float* o = img + (int64_t)b * NPART;
        const float I = o[3], D = o[4];
        const float W = use_dice ? kd * grad_scale * (has_grad_px ? o[7] : o[5] / (V + K_EPS)) : 0.f;
        o[0] = W * I / (D * D);
        o[1] = W * 2.f / D;
        o[2] = use_dice ? kd * (1.f - I / D) : 0.f;
    }
}

// per-pixel route: the dice value of the image joins every valid pixel of it
__global__ void mask_loss_px_dice_kernel(float* __restrict__ px, const int32_t* __restrict__ labels, const float* __restrict__ img, int64_t HW,
                                         int64_t P, int ignore) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < P; p += (int64_t)gridDim.x * blockDim.x)
        if (labels[p] != ignore) px[p] += img[(p / HW) * NPART + 2];
}

template <int SIG, bool DICE, int CE>
__global__ __launch_bounds__(256) void mask_loss_pass2_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int64_t HW,
                                                              int C, int ignore, int tpi, int pix, float ks_c, float kc, float w0, float w1,
                                                              const float* __restrict__ grad_px, const float* __restrict__ lse_px,
                                                              const float* __restrict__ img, const float* __restrict__ glob,
                                                              float* __restrict__ dlogits) {
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [pix][C]: logits in, gradient out
    const int64_t tl = blockIdx.x;
    const int64_t b = tl / tpi;
    const int64_t q0 = (tl - b * tpi) * pix;
    const int npx = (int)((HW - q0 < pix) ? (HW - q0) : pix);
    const int64_t p0 = b * HW + q0;
    const int64_t nel = (int64_t)npx * C;
    const bool vec = ((p0 * C) % 4 == 0) && (nel % 4 == 0);
    stage_in(tile, logits + p0 * C, nel, vec);
    __syncthreads();
    if ((int)threadIdx.x < npx) {
        float* z = tile + threadIdx.x * C;
        int y = labels[p0 + threadIdx.x];
        const bool keep = y != ignore;
        if (ignore == 0) y -= 1;
        const bool in_range = y >= 0 && y < C;
        if (!keep) {
            for (int c = 0; c < C; ++c) z[c] = 0.f;
        } else {
            const float g = glob[0] * (grad_px ? grad_px[p0 + threadIdx.x] : 1.f);
            const float gs = g * ks_c, gc = g * kc;
            const float cA = DICE ? img[b * NPART + 0] : 0.f, cB = DICE ? img[b * NPART + 1] : 0.f;
            const float zy = in_range ? z[y] : 0.f;
            const float lse = CE ? lse_px[p0 + threadIdx.x] : 0.f;
            // the CE gradient is k (delta_cy - softmax_c); plain CE: k = g k_c (and 0 for the zero one-hot row)
            float kce = 0.f;
            if (CE == 1) kce = in_range ? gc : 0.f;
            if (CE == 2 && in_range) {
                const float py = __expf(zy - lse);
                const float pc = fminf(fmaxf(py, 1e-7f), 1.f - 1e-7f);      // (read only where `live`: py inside the clip, never NaN)
                const float om = 1.f - pc;
                const float lg = __logf(pc);
                const bool live = py > 1e-7f && py < 1.f - 1e-7f;      // the clip passes no gradient outside its range
                // dl/dp = alpha (2 (1 - p) log p - (1 - p)^2 / p);   dp/dz_c = p (delta_cy - p_c)
                kce = live ? -gc * F_ALPHA * (2.f * om * lg - om * om / pc) * py : 0.f;
            }
            float d_y = 0.f;      // the t = 1 value of the label's class, from the untouched logit
            if (in_range) {
                if (SIG || DICE) {
                    const Sig q = sigmoid_parts<SIG == 2>(zy);
                    if (SIG == 1) d_y += gs * (q.s - 1.f);
                    if (SIG == 2) d_y -= gs * w1 * (q.oms * q.oms) * fmaf(2.f * q.s, q.bce0 - zy, q.oms);
                    if (DICE) d_y += q.s * q.oms * (cA - cB);
                }
                if (CE) d_y += kce * (__expf(zy - lse) - 1.f);
            }
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const float zc = z[c];
                float d = 0.f;
                if (SIG || DICE) {
                    const Sig q = sigmoid_parts<SIG == 2>(zc);
                    if (SIG == 1) d = gs * q.s;
                    if (SIG == 2) d = (gs * w0) * (q.s * q.s) * fmaf(2.f * q.oms, q.bce0, q.s);
                    if (DICE) d = fmaf(q.s * q.oms, cA, d);
                }
                if (CE) d = fmaf(kce, __expf(zc - lse), d);
                z[c] = d;
            }
            if (in_range) z[y] = d_y;
        }
    }
    __syncthreads();
    float* dst = dlogits + p0 * C;
    if (vec) {
        for (int i = threadIdx.x; i < nel / 4; i += 256) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<float4*>(tile)[i];
    } else {
        for (int i = threadIdx.x; i < nel; i += 256) dst[i] = tile[i];
    }
}

struct Layout {
    int pix, tpi;
    int64_t ntiles, P;
    size_t off_img, off_glob, off_lse, total;      // in floats
};

static inline Layout mask_loss_layout(int B, int64_t HW, int C) {
    Layout l;
    l.pix = mask_loss_pix(C);
    l.tpi = (int)ceil_div64(HW, l.pix);
    l.ntiles = (int64_t)B * l.tpi;
    l.P = (int64_t)B * HW;
    l.off_img = (size_t)l.ntiles * NPART;
    l.off_glob = l.off_img + (size_t)B * NPART;
    l.off_lse = l.off_glob + NPART;
    l.total = l.off_lse + (size_t)l.P;
    return l;
}

}  // namespace

extern "C" size_t iseg_mask_loss_workspace_bytes(int B, int64_t HW, int C) {
    if (B <= 0 || HW <= 0 || C <= 0) return 0;
    return mask_loss_layout(B, HW, C).total * sizeof(float);
}

extern "C" int iseg_mask_loss(const float* logits, const int32_t* labels, int B, int64_t HW, int C, int ignore_label, int flags,
                              float sigmoid_coef, float dice_coef, float ce_coef, float* loss_px, float* loss_mean, float loss_scale,
                              float* dlogits, float grad_scale, const float* grad_px, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(logits && labels && B > 0 && HW > 0 && C > 0, "iseg_mask_loss: bad arguments");
    ISEG_REQUIRE(C <= 256, "iseg_mask_loss: num_class %d > 256 unsupported (one 64-pixel tile of fp32 logits must fit 64 KiB of LDS)", C);
    ISEG_REQUIRE(flags & (ISEG_MASKLOSS_SIGMOID | ISEG_MASKLOSS_DICE | ISEG_MASKLOSS_CE), "iseg_mask_loss: no loss term enabled");
    ISEG_REQUIRE((int64_t)B * ceil_div64(HW, mask_loss_pix(C)) < (1ll << 31), "iseg_mask_loss: too many tiles");
    const Layout l = mask_loss_layout(B, HW, C);
    const size_t need = l.total * sizeof(float);
    ISEG_NEED_WORKSPACE("iseg_mask_loss", ws, ws_bytes, need);
    float* partials = (float*)ws;
    float* img = partials + l.off_img;
    float* glob = partials + l.off_glob;
    float* lse = partials + l.off_lse;
    const int sig = (flags & ISEG_MASKLOSS_SIGMOID) ? ((flags & ISEG_MASKLOSS_FOCAL_SIGMOID) ? 2 : 1) : 0;
    const int dice = (flags & ISEG_MASKLOSS_DICE) ? 1 : 0;
    const int ce = (flags & ISEG_MASKLOSS_CE) ? ((flags & ISEG_MASKLOSS_FOCAL_CE) ? 2 : 1) : 0;
    const bool bal = (flags & ISEG_MASKLOSS_CLASS_BALANCING) != 0;
    const float w0 = bal ? 1.f - F_ALPHA : 1.f, w1 = bal ? F_ALPHA : 1.f;
    const float ks_c = sigmoid_coef / (float)C;      // the mean over the classes
    const size_t lds = (size_t)l.pix * C * sizeof(float);
    const dim3 grid((unsigned)l.ntiles), block(256);
#define ML_LAUNCH(S, D, E)                                                                                                                    \
    do {                                                                                                                                      \
        hipLaunchKernelGGL((mask_loss_pass1_kernel<S, D, E>), grid, block, lds, stream, logits, labels, HW, C, ignore_label, l.tpi, l.pix,    \
                           ks_c, ce_coef, w0, w1, grad_px, loss_px, (E && dlogits) ? lse : (float*)nullptr, partials);                         \
        hipLaunchKernelGGL(mask_loss_finalize_kernel, dim3(1), dim3(1024), 0, stream, (const float*)partials, B, l.tpi, dice_coef, dice,      \
                           grad_px ? 1 : 0, grad_scale, loss_scale, img, glob, loss_mean);                                                     \
        if (loss_px && dice)                                                                                                                  \
            hipLaunchKernelGGL(mask_loss_px_dice_kernel, dim3(grid_cap(l.P, 256, 2048)),         \
                               dim3(256), 0, stream, loss_px, labels, (const float*)img, HW, l.P, ignore_label);                               \
        if (dlogits)                                                                                                                          \
            hipLaunchKernelGGL((mask_loss_pass2_kernel<S, D, E>), grid, block, lds, stream, logits, labels, HW, C, ignore_label, l.tpi,       \
                               l.pix, ks_c, ce_coef, w0, w1, grad_px, (const float*)lse, (const float*)img, (const float*)glob, dlogits);      \
    } while (0)
#define ML_CE(S, D)                       \
    do {                                  \
        if (ce == 0) ML_LAUNCH(S, D, 0);  \
        else if (ce == 1) ML_LAUNCH(S, D, 1); \
        else ML_LAUNCH(S, D, 2);          \
    } while (0)
#define ML_DICE(S)                 \
    do {                           \
        if (dice) ML_CE(S, true);  \
        else ML_CE(S, false);      \
    } while (0)
    if (sig == 0) ML_DICE(0);
    else if (sig == 1) ML_DICE(1);
    else ML_DICE(2);
#undef ML_DICE
#undef ML_CE
#undef ML_LAUNCH
    return iseg_check_launch("iseg_mask_loss");
}
