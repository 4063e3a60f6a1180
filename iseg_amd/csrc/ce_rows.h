// The row scheme of the per-pixel softmax kernels (loss.hip, ohem.hip): a workgroup stages `pix` pixels x C logits through LDS with fully
// coalesced 16-B lanes, each lane then owns one pixel (row stride C words; conflict-free for odd C such as 21).  Also the label-to-row rule
// of losses/catecrossentropy_ignore_label.py:56-61, so that every kernel that reads a label agrees on which pixels are zero rows.
#pragma once
#include "common.h"

static inline int pixels_per_block(int C) {
    int pix = (48 * 1024) / (4 * C);
    pix = (pix / 64) * 64;
    if (pix > 256) pix = 256;
    if (pix < 64) pix = 64;
    return pix;
}

// tile[0 .. nel) = src[0 .. nel), src = logits + first_el, by 256 threads; true when the 16-byte path was taken (the caller streams its
// result back out the same way)
__device__ __forceinline__ bool stage_rows(float* __restrict__ tile, const float* __restrict__ src, int64_t first_el, int64_t nel) {
    const bool vec = (first_el % 4 == 0) && (nel % 4 == 0);
    if (vec) {
        for (int i = threadIdx.x; i < nel / 4; i += 256) reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        for (int i = threadIdx.x; i < nel; i += 256) tile[i] = src[i];
    }
    return vec;
}

// y <- the class of tf.one_hot's row (ignore_label == 0 shifts every label down by one, :58-59); false when that row is the zero row
__device__ __forceinline__ bool label_class(int& y, int ignore, int C) {
    if (ignore == 0) y -= 1;
    return y >= 0 && y < C;
}
