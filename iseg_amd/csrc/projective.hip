// Batched projective transform: TensorFlow's ImageProjectiveTransformV3 in CONSTANT fill mode, the op behind RandomRotateAugment
// (augments/random_rotate_augment.py:20-115 transform, :221-296 random_rotated_inputs: bilinear image with fill -1 and
// tf.where(out < -1e-6, fill_constant_color, out), nearest label with fill = ignore label, one matrix for both).  One launch for a padded
// batch: a thread owns one output pixel, loops over the channels, reads at most 4 source pixels and writes the image pixel and the label, as
// augment_crop_kernel does; a workgroup owns a 32 x 8 tile of the output.  HBM-bound (reads <= 4 C floats + 1 label, writes 4 C + 4 B per pixel); no LDS, no atomics.
//
// Each sample has its own [8] row a0 a1 a2 b0 b1 b2 c0 c1 that maps the OUTPUT (x, y) to the INPUT (x', y'):
//   k = c0 x + c1 y + 1 (k == 0 -> fill);  x' = ((a0 x + a1 y) + a2) / k;  y' = ((b0 x + b1 y) + b2) / k
// in fp32, every product and sum rounded on its own (no FMA contraction): the nearest-neighbour label flips at a rounding boundary of x', so
// the coordinates have to be the bits a float32 restatement on the host computes.  The interpolation weights may contract.
// Bounds are tested on the FLOAT coordinate (rounded or floored) before any conversion to int: huge, infinite and NaN coordinates are out
// of bounds.  One departure from TF's arithmetic, only visible at |x'| >= 2^24: where none of the four bilinear taps is inside the sample
// the result is the fill value itself (TF's fp32 weights xc - x' and x' - xf both collapse to 0 there and it returns 0).
#include "common.h"
#include "iseg_hip.h"

namespace {

struct ProjConst {
    float replace[4];
    int has_replace;
};

constexpr int TILE_W = 32, TILE_H = 8;      // 256 threads

__device__ __forceinline__ bool source_xy(const float* __restrict__ t, float x, float y, float& sx, float& sy) {
#pragma clang fp contract(off)
    const float k = (t[6] * x + t[7] * y) + 1.f;
    if (k == 0.f) return false;
    sx = ((t[0] * x + t[1] * y) + t[2]) / k;
    sy = ((t[3] * x + t[4] * y) + t[5]) / k;
    return true;
}

template <int C, int INTERP>
__global__ __launch_bounds__(256) void projective_kernel(const float* __restrict__ img, const int32_t* __restrict__ lab,
                                                         const float* __restrict__ transforms, const int32_t* __restrict__ sizes,
                                                         float* __restrict__ out_img, int32_t* __restrict__ out_lab, int B, int Hs, int Ws,
                                                         float fill, ProjConst k, int label_fill) {
    // a workgroup owns a TILE_W x TILE_H output tile (a wavefront: TILE_W x 2), not 256 pixels of one row: under a rotation a row of
    // outputs reads along a slanted line that meets a new cache line every few pixels, a tile reads a compact rotated rectangle
    const int tiles_x = (Ws + TILE_W - 1) / TILE_W, tiles_y = (Hs + TILE_H - 1) / TILE_H;
    const int64_t tiles = (int64_t)B * tiles_y * tiles_x;
    const int tx = (int)threadIdx.x % TILE_W, ty = (int)threadIdx.x / TILE_W;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x = (int)(tile % tiles_x) * TILE_W + tx, y = (int)((tile / tiles_x) % tiles_y) * TILE_H + ty;
        const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
        if (x >= Ws || y >= Hs) continue;
        const int64_t i = ((int64_t)b * Hs + y) * Ws + x;
        // the sample's own size inside the padded buffer (clamped: a bad table can never index outside it)
        const int H = sizes ? min(max(sizes[2 * b], 0), Hs) : Hs, W = sizes ? min(max(sizes[2 * b + 1], 0), Ws) : Ws;
        float v[C];
        int l = label_fill;
        if (y >= H || x >= W) {      // padding of the batch buffer
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = k.has_replace ? k.replace[c] : fill;
        } else {
            const float* src = img + (int64_t)b * Hs * Ws * C;
            const float fH = (float)H, fW = (float)W;
            float sx = 0.f, sy = 0.f;
            const bool ok = source_xy(transforms + (int64_t)b * 8, (float)x, (float)y, sx, sy);
            // nearest: (lround(y'), lround(x')), half away from zero
            const float rx = roundf(sx), ry = roundf(sy);
            const bool inside = ok && rx >= 0.f && rx < fW && ry >= 0.f && ry < fH;
            const int64_t npix = inside ? (int64_t)(int)ry * Ws + (int)rx : 0;
            if (lab && inside) l = lab[(int64_t)b * Hs * Ws + npix];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = fill;
            if (INTERP == 0) {
                if (inside) {
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c] = src[npix * C + c];
                }
            } else if (ok) {
                const float xf = floorf(sx), yf = floorf(sy), xc = xf + 1.f, yc = yf + 1.f;
                const bool x0 = xf >= 0.f && xf < fW, x1 = xc >= 0.f && xc < fW, y0 = yf >= 0.f && yf < fH, y1 = yc >= 0.f && yc < fH;
                if ((x0 || x1) && (y0 || y1)) {
                    const float wx0 = xc - sx, wx1 = sx - xf, wy0 = yc - sy, wy1 = sy - yf;
                    // (an index is formed only where its tap is inside; the others are never read)
                    const int64_t r0 = y0 ? (int64_t)(int)yf * Ws : 0, r1 = y1 ? (int64_t)(int)yc * Ws : 0;
                    const int64_t c0 = x0 ? (int)xf : 0, c1 = x1 ? (int)xc : 0;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float p00 = y0 && x0 ? src[(r0 + c0) * C + c] : fill, p01 = y0 && x1 ? src[(r0 + c1) * C + c] : fill;
                        const float p10 = y1 && x0 ? src[(r1 + c0) * C + c] : fill, p11 = y1 && x1 ? src[(r1 + c1) * C + c] : fill;
                        const float top = wx0 * p00 + wx1 * p01, bot = wx0 * p10 + wx1 * p11;
                        v[c] = wy0 * top + wy1 * bot;
                    }
                }
            }
            if (k.has_replace) {      // the reference's tf.where(out < 0 - 1e-6, fill_constant_color, out)
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = v[c] < -1e-6f ? k.replace[c] : v[c];
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out_img[i * C + c] = v[c];
        if (out_lab) out_lab[i] = l;
    }
}

template <int C>
void launch(int interp, unsigned blocks, hipStream_t stream, const float* images, const int32_t* labels, const float* transforms,
            const int32_t* sizes, float* out_images, int32_t* out_labels, int B, int Hs, int Ws, float fill, const ProjConst& k, int label_fill) {
    if (interp == 0)
        hipLaunchKernelGGL((projective_kernel<C, 0>), dim3(blocks), dim3(256), 0, stream, images, labels, transforms, sizes, out_images,
                           out_labels, B, Hs, Ws, fill, k, label_fill);
    else
        hipLaunchKernelGGL((projective_kernel<C, 1>), dim3(blocks), dim3(256), 0, stream, images, labels, transforms, sizes, out_images,
                           out_labels, B, Hs, Ws, fill, k, label_fill);
}

}  // namespace

extern "C" int iseg_projective_transform_batch(const float* images, const int32_t* labels, const float* transforms, const int32_t* sizes,
                                               float* out_images, int32_t* out_labels, int B, int Hs, int Ws, int C, int image_interp,
                                               float image_fill, const float* replace, int label_fill, hipStream_t stream) {
    ISEG_REQUIRE(images && transforms && out_images && B > 0 && Hs > 0 && Ws > 0, "iseg_projective_transform_batch: bad arguments");
    ISEG_REQUIRE((labels != nullptr) == (out_labels != nullptr), "iseg_projective_transform_batch: labels and out_labels go together");
    if (C < 1 || C > 4 || (image_interp != 0 && image_interp != 1) || Hs > (1 << 24) || Ws > (1 << 24)) {
        iseg_set_error("iseg_projective_transform_batch: C in 1..4, image_interp 0 (nearest) or 1 (bilinear), Hs, Ws <= 2^24; got C %d, interp %d, "
                       "%d x %d", C, image_interp, Hs, Ws);
        return ISEG_ERR_UNSUPPORTED;
    }
    ProjConst k{};
    k.has_replace = replace != nullptr;
    for (int c = 0; c < C && replace; ++c) k.replace[c] = replace[c];
    const int64_t tiles = (int64_t)B * ceil_div64(Hs, TILE_H) * ceil_div64(Ws, TILE_W);
    const unsigned blocks = grid_cap(tiles, 1, 16384);
    switch (C) {
        case 1: launch<1>(image_interp, blocks, stream, images, labels, transforms, sizes, out_images, out_labels, B, Hs, Ws, image_fill, k, label_fill); break;
        case 2: launch<2>(image_interp, blocks, stream, images, labels, transforms, sizes, out_images, out_labels, B, Hs, Ws, image_fill, k, label_fill); break;
        case 3: launch<3>(image_interp, blocks, stream, images, labels, transforms, sizes, out_images, out_labels, B, Hs, Ws, image_fill, k, label_fill); break;
        default: launch<4>(image_interp, blocks, stream, images, labels, transforms, sizes, out_images, out_labels, B, Hs, Ws, image_fill, k, label_fill); break;
    }
    return iseg_check_launch("iseg_projective_transform_batch");
}
