// Connected-components labelling (ops/ccl.py of the reference: label_components :28-36, _label_components :46-54, find_components :65-103,
// search :117-160, search_neighbors :172-214).  mask [N,H,W] -> labels [N,H,W] int32, image by image: background 0, every foreground pixel the
// number of its 4-connected component (neighbours up, left, right, down: NEIGHBORS_COORDS :11-16; a neighbour outside the image is masked out,
// :188-201, so rows do not wrap), components numbered 1, 2, 3, ... in the raster order of their first pixel (the loop over i with label += 1 at
// every still unlabelled pixel, :75-92).  The reduce_sum <= 1 shortcut (:48-54) returns the input, which IS the labelling of such an image.
// One decision beyond the reference: ANY non-zero mask value is foreground (int32 {0,1}, and uint8 / bool masks with 0 / 255).  The reference
// hands a pixel that is neither 0 nor 1 back negated (-binary_img is only ever compared with -1, :52, :80), which is no labelling.
//
// The reference is a serial flood fill.  This is a union-find over pixels that always links the larger root under the smaller one, so a
// component ends up rooted at its smallest linear index y * W + x -- its first raster pixel -- and its number is 1 + the count of roots
// with a smaller index.
//
// Encoding.  `labels` is the parent array: a foreground pixel p (index inside its image) holds parent + 1, a root holds p + 1, background 0;
// a parent is never larger than its child.  From the rank pass on a root holds -(number); finalise turns every entry into the number.
//
//   local     one workgroup per 64 x 16 tile (a tile row is one wavefront: 256-byte rows of labels).  Horizontal runs come from a ballot (every
//             pixel starts under its run's first pixel, no atomics); vertical links are LDS atomicMin on roots; every pixel then stores the
//             image index of its tile-local root + 1.
//   seam      one workgroup per tile, over its first row and first column: union across the tile border in global memory, lock-free
//             (atomicMin on the larger root; if it was no root any more, go on from what it held).  Every read of a parent bypasses the L1.
//   flatten   one workgroup per image row: every pixel walks to its root and stores root + 1; the row's root count goes to row_base.
//   scan      one workgroup per image: row_base -> its exclusive prefix; counts[n] = the total.
//   rank      one workgroup per image row: in-row prefix over the root flags; a root becomes -(row_base + prefix + 1).
//   finalise  one workgroup per image row: v < 0 -> -v;  v > 0 -> |labels[v - 1]| (a root: -number, or +number if its own thread came first).
//
// Integer atomics only, no floating point, exact grids (N on a grid axis).  No thread waits for another workgroup: every loop either walks
// a parent chain (the index strictly decreases), replaces the larger of two roots by something smaller, or counts a row's columns.
// No host read, no copy, no allocation: the call captures into a graph.
#include "common.h"
#include "iseg_hip.h"

namespace {

constexpr int TW = 64, TH = 16;      // tile: one wavefront per row, four rows per wavefront
typedef unsigned long long u64;

// ---- LDS union-find over tile-local indices ly * 64 + lx -------------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(const int* s, int i) { return __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(const int* s, int x) {
    for (int p = lds_load(s, x); p != x; p = lds_load(s, x)) x = p;      // p < x
    return x;
}

__device__ __forceinline__ void lds_union(int* s, int a, int b) {
    for (;;) {
        a = lds_find(s, a);
        b = lds_find(s, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(s + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;      // a was a root and now hangs under b
        a = old;                   // a had a parent old < a: whichever of old and b it lost, join that one with b
    }
}

template <bool U8> __device__ __forceinline__ bool mask_at(const void* mask, int64_t i) {
    return U8 ? ((const uint8_t*)mask)[i] != 0 : ((const int32_t*)mask)[i] != 0;
}

template <bool U8>
__global__ __launch_bounds__(256) void ccl_local_kernel(const void* __restrict__ mask, int H, int W, int32_t* __restrict__ labels) {
    __shared__ int s[TW * TH];
    __shared__ u64 rows[TH];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, gx = x0 + lane;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    const u64 below = ((u64)1 << lane) - 1;
    bool fg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = wid * 4 + k, gy = y0 + ly;
        fg[k] = gx < W && gy < H && mask_at<U8>(mask, img + (int64_t)gy * W + gx);
        const u64 m = __ballot(fg[k]);
        const u64 gaps = ~m & below;      // background lanes left of this one: the run starts right of the last of them
        const int start = gaps ? 64 - __clzll(gaps) : 0;
        s[ly * TW + lane] = fg[k] ? ly * TW + start : -1;
        if (lane == 0) rows[ly] = m;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = wid * 4 + k;
        if (ly == 0 || !fg[k]) continue;
        const u64 m = rows[ly], up = rows[ly - 1];
        // the link to the pixel above is implied where left and upper-left are both set: p ~ left (same run), left ~ upper-left, upper-left ~ up
        const bool implied = lane > 0 && ((m & up) >> (lane - 1) & 1);
        if ((up >> lane & 1) && !implied) lds_union(s, ly * TW + lane, (ly - 1) * TW + lane);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = wid * 4 + k, gy = y0 + ly;
        if (gx >= W || gy >= H) continue;
        int v = 0;
        if (fg[k]) {
            const int r = lds_find(s, ly * TW + lane);
            v = (y0 + r / TW) * W + x0 + r % TW + 1;
        }
        labels[img + (int64_t)gy * W + gx] = v;
    }
}

// ---- global union-find over image indices; L[p] = parent + 1 --------------------------------------------------------------------------
__device__ __forceinline__ int glb_load(const int32_t* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int glb_find(const int32_t* L, int x) {
    for (int p = glb_load(L, x) - 1; p != x; p = glb_load(L, x) - 1) x = p;      // p < x
    return x;
}

__device__ __forceinline__ void glb_union(int32_t* L, int a, int b) {
    for (;;) {
        a = glb_find(L, a);
        b = glb_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(L + a, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
        if (old == a) return;
        a = old;
    }
}

// lanes 0..63: the tile's first row against the row above; lanes 64..79: its first column against the column to the left
__global__ __launch_bounds__(128) void ccl_seam_kernel(int H, int W, int32_t* labels) {
    int32_t* L = labels + (int64_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, t = threadIdx.x;
    if (t < TW) {
        const int x = x0 + t;
        if (y0 == 0 || x >= W) return;
        const int p = y0 * W + x, q = p - W;
        if (glb_load(L, p) == 0 || glb_load(L, q) == 0) return;
        // implied where left and upper-left are both set (see ccl_local_kernel; the links it leans on are made by somebody, in any order)
        if (x > 0 && glb_load(L, p - 1) != 0 && glb_load(L, q - 1) != 0) return;
        glb_union(L, p, q);
    } else if (t < TW + TH) {
        const int y = y0 + (t - TW);
        if (x0 == 0 || y >= H) return;
        const int p = y * W + x0;
        if (glb_load(L, p) == 0 || glb_load(L, p - 1) == 0) return;
        glb_union(L, p, p - 1);
    }
}

// sum of one flag per thread over the workgroup's four wavefronts
__device__ __forceinline__ int block_count_256(bool flag, int* red) {
    const int c = __popcll(__ballot(flag));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void ccl_flatten_kernel(int H, int W, int32_t* labels, int32_t* __restrict__ row_base) {
    __shared__ int red[4];
    int32_t* L = labels + (int64_t)blockIdx.y * H * W;
    const int y = blockIdx.x;
    int roots = 0;
    for (int xb = 0; xb < W; xb += 256) {
        const int x = xb + threadIdx.x, p = y * W + x;
        bool root = false;
        if (x < W) {
            const int v = L[p];
            if (v > 0) {
                int r = v - 1;
                // other walkers store root + 1 over parent + 1 meanwhile: either value is an ancestor, and a root's own entry never changes
                for (int q = L[r] - 1; q != r; q = L[r] - 1) r = q;      // q < r
                root = r == p;
                if (r + 1 != v) L[p] = r + 1;
            }
        }
        roots += block_count_256(root, red);
    }
    if (threadIdx.x == 0) row_base[(int64_t)blockIdx.y * H + y] = roots;
}

// row_base[n, :] -> its exclusive prefix; counts[n] = the sum.  Thread t owns the rows t * per .. (t + 1) * per - 1.
__global__ __launch_bounds__(256) void ccl_scan_kernel(int H, int32_t* __restrict__ row_base, int32_t* __restrict__ counts) {
    __shared__ int s[256];
    int32_t* rb = row_base + (int64_t)blockIdx.x * H;
    const int t = threadIdx.x, per = (H + 255) / 256, r0 = min(H, t * per), r1 = min(H, r0 + per);
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += rb[r];
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int run = s[t] - sum;
    for (int r = r0; r < r1; ++r) {
        const int c = rb[r];
        rb[r] = run;
        run += c;
    }
    if (t == 255) counts[blockIdx.x] = s[255];
}

__global__ __launch_bounds__(256) void ccl_rank_kernel(int H, int W, int32_t* __restrict__ labels, const int32_t* __restrict__ row_base) {
    __shared__ int red[4];
    int32_t* L = labels + (int64_t)blockIdx.y * H * W;
    const int y = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int base = row_base[(int64_t)blockIdx.y * H + y];
    for (int xb = 0; xb < W; xb += 256) {
        const int x = xb + threadIdx.x, p = y * W + x;
        const bool root = x < W && L[p] == p + 1;
        const u64 m = __ballot(root);
        __syncthreads();
        if (lane == 0) red[wid] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & (((u64)1 << lane) - 1));
        for (int w = 0; w < wid; ++w) before += red[w];
        if (root) L[p] = -(base + before + 1);
        base += (red[0] + red[1]) + (red[2] + red[3]);
    }
}

__global__ __launch_bounds__(256) void ccl_finalize_kernel(int H, int W, int32_t* labels) {
    int32_t* L = labels + (int64_t)blockIdx.y * H * W;
    const int y = blockIdx.x;
    for (int x = threadIdx.x; x < W; x += 256) {
        const int p = y * W + x, v = L[p];
        if (v < 0) L[p] = -v;
        else if (v > 0) L[p] = abs(L[v - 1]);
    }
}

}  // namespace

extern "C" int iseg_ccl_label(const void* mask, int mask_is_u8, int N, int H, int W, int32_t* labels, int32_t* counts, int32_t* row_base,
                              hipStream_t stream) {
    ISEG_REQUIRE(mask && labels && counts && row_base, "iseg_ccl_label: null mask, labels, counts or row_base");
    ISEG_REQUIRE(N >= 1 && N <= 65535, "iseg_ccl_label: %d images per call (1..65535)", N);
    ISEG_REQUIRE(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "iseg_ccl_label: a %d x %d image (1..16384 a side: H * W + 1 is an int32)", H, W);
    ISEG_REQUIRE(mask != (const void*)labels, "iseg_ccl_label: labels is the parent array while the mask is read, it cannot be the mask");
    const dim3 tiles((W + TW - 1) / TW, (H + TH - 1) / TH, N), rows(H, N);
    if (mask_is_u8) hipLaunchKernelGGL((ccl_local_kernel<true>), tiles, dim3(256), 0, stream, mask, H, W, labels);
    else hipLaunchKernelGGL((ccl_local_kernel<false>), tiles, dim3(256), 0, stream, mask, H, W, labels);
    if (tiles.x > 1 || tiles.y > 1) hipLaunchKernelGGL(ccl_seam_kernel, tiles, dim3(128), 0, stream, H, W, labels);
    hipLaunchKernelGGL(ccl_flatten_kernel, rows, dim3(256), 0, stream, H, W, labels, row_base);
    hipLaunchKernelGGL(ccl_scan_kernel, dim3(N), dim3(256), 0, stream, H, row_base, counts);
    hipLaunchKernelGGL(ccl_rank_kernel, rows, dim3(256), 0, stream, H, W, labels, (const int32_t*)row_base);
    hipLaunchKernelGGL(ccl_finalize_kernel, rows, dim3(256), 0, stream, H, W, labels);
    return iseg_check_launch("iseg_ccl_label");
}
