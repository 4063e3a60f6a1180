// Depthwise 7 x 7 weight gradient (stride 1, dilation 1, bf16 storage, C % 32 == 0) on the matrix cores.
//     dW[ky][kx][c] = sum_{n,r,q} Xp[n][r + ky][q + kx][c] dY[n][r][q][c]        db[c] = sum dY[n][r][q][c]        (Xp: the zero-padded input)
// Same instruction and block = channel mapping as dwconv_mfma.hip (v_mfma_f32_4x4x4_16b_bf16: sixteen independent 4 x 4 x 4 products).  One MFMA
// takes an output column q, a chunk of four padded input rows rho0 = 4 chunk, a kernel-column group kx0 in {0, 4} and a kernel-row group ky0 in
// {0, 4}:
//     A_b[m][k] = Xp[rho0 + k][q + kx0 + m]               (lane 4b + m: 8 bytes of the planar image, as dwconv7_mfma_kernel reads them)
//     B_b[k][n] = dY[rho0 + k - (ky0 + n)][q] = dY[4 j + k - n][q],   j = chunk - ky0 / 4        (zero outside the tile's 16 rows)
//     D_b[m][n] += A_b B_b = partial dW[ky0 + n][kx0 + m]   (lane 4b + n, register m)
// Four 4 x 4 patches = 16 accumulator registers per lane hold the 8 x 8 superset of the 7 x 7 taps (row / column 7 discarded) and persist over
// all tiles of the workgroup.  B depends on chunk and ky0 only through j; j = -1 and j = 5 are all zero, so a (q, 16 channels) costs 5 B
// fragments, 12 A fragments and 20 MFMAs (49 of 64 products per MFMA carry a tap).
//
// Shifted B fragments.  Lane n wants rows 4 j - n ..: an 8-byte read at a 2-byte granular offset.  The dY plane is kept as TWO planar copies
// E_s[t] = dY[t - 2 - s], s = n & 1; lane n reads copy n & 1 at t = 4 j + 2 - 2 (n >> 1), which is even: a 4-byte aligned ds_read2_b32.  Both
// copies come straight out of the transposing read of the raw dY tile (its row origin moved by 2 + s rows): no register shuffling.
//
// Unit = (16-channel slab, image, 16 x 16 dY tile).  A 16-channel slab halves every LDS image against dwconv7_mfma_kernel's 32: 74 KB per workgroup
// of four wavefronts, so TWO workgroups per CU overlap each other's phases; the slabs of one tile run on the same XCD and share its 128-byte lines
// in L2.  Per unit:
//   HBM --global_load_lds--> raw NHWC tiles: x [24 rows][22 columns][16 ch] (17 KiB-pieces), dY [16][18][16] (9 pieces; 3 zero rows above, 2 below,
//       written once)
//       --ds_read_b64_tr_b16 / ds_write_b64--> planar x P[16][22 columns][28 rows] (36 tasks), planar dY E_0, E_1 [16][16 columns][24] (40 tasks);
//       the copy-0 tasks also add their four rows into the bias gradient (every dY element exactly once)
//   the raw tiles are dead now: the NEXT unit's DMA is issued here and lands under the products
//   wavefront w: columns 4 w .. 4 w + 3, all 16 channels: 4 x (17 fragment reads, 20 MFMAs) as four independent accumulator chains.
// Wavefronts -> workgroup by a fixed-order sum in LDS, workgroups -> result by launch_reduce_rows: no atomics, bit-reproducible.
#include "common.h"
#include "dwconv_mfma_common.h"
#include "iseg_hip.h"

namespace {

using dwm::f32x4_t;
using dwm::s16x4;
using dwm::u32x2_t;

__device__ uint4 wgm_zero_page[2];      // 32 zero bytes (device globals are zero-initialised)

constexpr int TR = 16, TC = 16, CH = 16, KS = 7, NT = KS * KS + 1, WAVES = 4;
constexpr int X_ROWS = 24, X_COLS = 22, X_PITCH = 22;      // pixels of 32 B; 22 x 8 dwords == 48 mod 64: the four rows of a transposing read on distinct banks
constexpr int X_PIECES = (X_ROWS * X_PITCH + 31) / 32;     // 17 one-KiB pieces (32 pixels each)
constexpr int D_PITCH = 18, D_PIECES = TR * D_PITCH / 32;  // 18 x 8 == 16 mod 64; rows 0 .. 15 are exactly 9 pieces
constexpr int D_TOP = 2048, D_BOT = 2048;                  // zero rows -3 .. -1 (1728 B) above and 16, 17 (1152 B) below the DMA'd rows
static_assert(TR * D_PITCH % 32 == 0 && 3 * D_PITCH * 32 <= D_TOP && 2 * D_PITCH * 32 <= D_BOT, "dY tile layout");
constexpr int PLANE = 1248, COLP = 56;                     // planar x: bytes per channel plane / per column (28 rows), as dwconv_mfma.hip
constexpr int E_COL = 48, E_PLANE = TC * E_COL + 16, E_COPY = CH * E_PLANE + 128;      // planar dY: plane == 4 banks mod 64, copy 1 half a bank cycle away
constexpr int RX_OFF = 0, RD_OFF = RX_OFF + X_PIECES * 1024, PX_OFF = RD_OFF + D_TOP + D_PIECES * 1024 + D_BOT, PE_OFF = PX_OFF + CH * PLANE;
constexpr int LDS_BYTES = PE_OFF + 2 * E_COPY;
constexpr int X_TASKS = 6 * 6, E_TASKS = 2 * 5 * 4;        // (row chunk, column quad) / (copy, row chunk, column quad)
constexpr int NPX = (X_PIECES + WAVES - 1) / WAVES, NPD = (D_PIECES + WAVES - 1) / WAVES;
static_assert(X_COLS * COLP <= PLANE && LDS_BYTES <= 80 * 1024 && PX_OFF % 8 == 0 && PE_OFF % 8 == 0, "two workgroups per CU");
static_assert(WAVES * NT * CH * 4 + WAVES * 4 * CH * 4 <= LDS_BYTES, "final reduction fits");

// One dY column q = 4 wid + QI of 16 channels: twelve A fragments (6 row chunks x 2 kernel-column groups), five B fragments, 20 MFMAs as four
// independent accumulator chains.  acc[ky0 / 4][kx0 / 4]: lane (channel, n), register m = dW[ky0 + n][kx0 + m].
template <int QI>
__device__ __forceinline__ void wgm_column(unsigned a_base, unsigned b_base, f32x4_t (&acc)[2][2]) {
    u32x2_t a[2][6], b[5];
#define WGM_RDA(G, CK) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(a[G][CK]) : "v"(a_base), "n"((QI + 4 * (G)) * COLP + (CK) * 8) : "memory")
#define WGM_RDB(J) \
    asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(b[J]) : "v"(b_base), "n"(QI * (E_COL / 4) + 2 * (J)), "n"(QI * (E_COL / 4) + 2 * (J) + 1) : "memory")
    WGM_RDB(0); WGM_RDA(0, 0); WGM_RDA(1, 0); WGM_RDA(0, 1); WGM_RDA(1, 1);
    WGM_RDB(1); WGM_RDA(0, 2); WGM_RDA(1, 2);
    WGM_RDB(2); WGM_RDA(0, 3); WGM_RDA(1, 3);
    WGM_RDB(3); WGM_RDA(0, 4); WGM_RDA(1, 4);
    WGM_RDB(4); WGM_RDA(0, 5); WGM_RDA(1, 5);
#undef WGM_RDA
#undef WGM_RDB
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[0][3]), "+v"(a[0][4]), "+v"(a[0][5]), "+v"(a[1][0]),
                 "+v"(a[1][1]), "+v"(a[1][2]), "+v"(a[1][3]), "+v"(a[1][4]), "+v"(a[1][5]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4])
                 :: "memory");
#pragma unroll
    for (int j = 0; j < 5; ++j) {      // B_j meets row chunk j for ky0 = 0 and row chunk j + 1 for ky0 = 4
        const s16x4 bj = __builtin_bit_cast(s16x4, b[j]);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            acc[0][g] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(s16x4, a[g][j]), bj, acc[0][g], 0, 0, 0);
            acc[1][g] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(s16x4, a[g][j + 1]), bj, acc[1][g], 0, 0, 0);
        }
    }
}

__global__ __launch_bounds__(64 * WAVES, 2) void dwconv7_wgrad_mfma_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                                          float* __restrict__ partials, int N, int H, int W, int C, int pad_t,
                                                                          int pad_l, int tiles_h, int tiles_w, int tiles_per_wg) {
    extern __shared__ __attribute__((aligned(1024))) char smem_wgm[];
    const unsigned lds0 = (unsigned)(uintptr_t)(dwm::lds_ptr)smem_wgm;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = blockIdx.y * CH;
    const int ntiles = N * tiles_h * tiles_w;
    // blockIdx.x round-robins over the 8 XCDs: give each XCD a contiguous run of the tile sequence (neighbouring tiles share halo in its L2; the
    // slabs of a tile, same blockIdx.x, meet on one XCD)
    int lb = blockIdx.x;
    if (gridDim.x % 8 == 0) lb = (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
    const int t_begin = min(ntiles, lb * tiles_per_wg), t_end = min(ntiles, t_begin + tiles_per_wg);

    // ---- once: the constant zeros of the LDS images (dY rows outside the tile, planar dY entries t = 20 .. 23) ----
    for (int i = tid; i < (D_TOP + D_BOT) / 8; i += 64 * WAVES) {
        const int o = i * 8 < D_TOP ? i * 8 : D_TOP + D_PIECES * 1024 + (i * 8 - D_TOP);
        *reinterpret_cast<uint2*>(smem_wgm + RD_OFF + o) = make_uint2(0u, 0u);
    }
    for (int i = tid; i < 2 * CH * TC; i += 64 * WAVES) {
        const int s = i / (CH * TC), ch = (i / TC) % CH, col = i % TC;
        *reinterpret_cast<uint2*>(smem_wgm + PE_OFF + s * E_COPY + ch * E_PLANE + col * E_COL + 40) = make_uint2(0u, 0u);
    }

    // ---- per-lane constants ----
    // DMA: piece p = wid + 4 i covers pixels 32 p .. 32 p + 31, lane -> (pixel 32 p + lane / 2, 8-channel half lane % 2); (row, column) of the pixel
    // within the tile does not depend on the tile.  Rows 22, 23 of the x tile and the two pad columns of the dY tile read the zero page.
    int xrc[NPX], drc[NPD];
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        const int pix = (wid + WAVES * i) * 32 + (lane >> 1);
        const int rr = pix / X_PITCH, cc = pix - rr * X_PITCH;
        xrc[i] = ((rr >= TR + KS - 1 ? 0x7fff : rr) << 16) | cc;
    }
#pragma unroll
    for (int i = 0; i < NPD; ++i) {
        const int pix = (wid + WAVES * i) * 32 + (lane >> 1);
        const int rr = pix / D_PITCH, cc = pix - rr * D_PITCH;
        drc[i] = ((cc >= TC || rr >= TR ? 0x7fff : rr) << 16) | cc;
    }
    const bf16_t* const zero = reinterpret_cast<const bf16_t*>(wgm_zero_page) + (lane & 1) * 8;
    auto issue_dma = [&](int tile) {
        int b = tile;
        const int tw_i = b % tiles_w;
        b /= tiles_w;
        const int th_i = b % tiles_h;
        const int n = b / tiles_h;
        const int h0 = th_i * TR, w0 = tw_i * TC;
        const bf16_t* xb = x + (((n * H + h0 - pad_t) * W + w0 - pad_l) * C + c0 + (lane & 1) * 8);      // (may point before the image: only used under `ok`)
        const bf16_t* db = dy + (((n * H + h0) * W + w0) * C + c0 + (lane & 1) * 8);
#pragma unroll
        for (int i = 0; i < NPX; ++i) {
            const int p = wid + WAVES * i;
            if (p < X_PIECES) {      // wavefront-uniform
                int rc = xrc[i];
                asm volatile("" : "+v"(rc));      // one register per piece (keeps hipcc from hoisting every derived offset out of the tile loop)
                const int rr = rc >> 16, cc = rc & 0xffff;
                const bool ok = (unsigned)(h0 - pad_t + rr) < (unsigned)H && (unsigned)(w0 - pad_l + cc) < (unsigned)W;
                const bf16_t* src = ok ? xb + __mul24(__mul24(rr, W) + cc, C) : zero;
                __builtin_amdgcn_global_load_lds((dwm::glb_ptr)src, (dwm::lds_ptr)(smem_wgm + RX_OFF + p * 1024), 16, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < NPD; ++i) {
            const int p = wid + WAVES * i;
            if (p < D_PIECES) {
                int rc = drc[i];
                asm volatile("" : "+v"(rc));
                const int rr = rc >> 16, cc = rc & 0xffff;
                const bool ok = (unsigned)(h0 + rr) < (unsigned)H && (unsigned)(w0 + cc) < (unsigned)W;
                const bf16_t* src = ok ? db + __mul24(__mul24(rr, W) + cc, C) : zero;
                __builtin_amdgcn_global_load_lds((dwm::glb_ptr)src, (dwm::lds_ptr)(smem_wgm + RD_OFF + D_TOP + p * 1024), 16, 0, 0);
            }
        }
    };
    // transposition: lane (g = lane / 16, q = (lane / 4) % 4, p = lane % 4) reads raw[row0 + q][4 cq + g][4 p .. 4 p + 3]; afterwards lane
    // (g, i = lane % 16) holds rows row0 .. row0 + 3 of channel i at column 4 cq + g
    const int tg = lane >> 4, ti = lane & 15;
    const unsigned trx_src = lds0 + RX_OFF + (((ti >> 2) * X_PITCH) + tg) * 32 + (ti & 3) * 8;
    const unsigned trx_dst = lds0 + PX_OFF + ti * PLANE + tg * COLP;
    const unsigned trd_src = lds0 + RD_OFF + D_TOP + (((ti >> 2) * D_PITCH) + tg) * 32 + (ti & 3) * 8;
    const unsigned trd_dst = lds0 + PE_OFF + ti * E_PLANE + tg * E_COL;
    // products: wavefront -> columns 4 wid .. 4 wid + 3, lane -> (channel chl, m / n = lane % 4)
    const int chl = lane >> 2, mn = lane & 3;
    const unsigned a_base = lds0 + PX_OFF + chl * PLANE + (4 * wid + mn) * COLP;
    const unsigned b_base = lds0 + PE_OFF + (mn & 1) * E_COPY + chl * E_PLANE + (4 * wid) * E_COL + 4 - 4 * (mn >> 1);

    f32x4_t acc[2][2];      // [ky0 / 4][kx0 / 4]: lane (chl, n), register m = dW[ky0 + n][kx0 + m]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float accb = 0.f;      // lane (g, i): bias-gradient share of channel i (columns == g mod 4, this wavefront's tasks)

    if (t_begin < t_end) issue_dma(t_begin);
    for (int tile = t_begin; tile < t_end; ++tile) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this tile has landed
        __syncthreads();                                       // ... for every wavefront; the previous tile's planar images are consumed

        // ---- raw -> planar (transposing reads) ----
        {
            u32x2_t tv[9] = {};
#pragma unroll
            for (int i = 0; i < 9; ++i) {      // x: task = (row chunk R, column quad cq) = wid + 4 i, 36 of them
                const int task = wid + WAVES * i, R = task / 6, cq = task - R * 6;
                dwm::lds_read_tr16_b64(tv[i], trx_src + (4 * R * X_PITCH + 4 * cq) * 32);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]), "+v"(tv[5]), "+v"(tv[6]), "+v"(tv[7]), "+v"(tv[8])
                         :: "memory");
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const int task = wid + WAVES * i, R = task / 6, cq = task - R * 6;
                if (4 * cq + tg < X_COLS)      // (columns 22, 23 of the last quad do not exist: their lanes read the next row's pixels and drop them)
                    asm volatile("ds_write_b64 %0, %1" ::"v"(trx_dst + (4 * cq) * COLP + R * 8), "v"(tv[i]) : "memory");
            }
        }
        {
            u32x2_t tv[10] = {};
#pragma unroll
            for (int i = 0; i < 10; ++i) {      // dY: task = (copy s, row chunk T, column quad cq) = wid + 4 i, 40 of them; E_s[4 T + k] = dY[4 T - 2 - s + k]
                const int task = wid + WAVES * i, s = task / 20, T = (task / 4) % 5, cq = task & 3;
                dwm::lds_read_tr16_b64(tv[i], trd_src + ((4 * T - 2 - s) * D_PITCH + 4 * cq) * 32);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]), "+v"(tv[4]), "+v"(tv[5]), "+v"(tv[6]), "+v"(tv[7]), "+v"(tv[8]),
                         "+v"(tv[9]) :: "memory");
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const int task = wid + WAVES * i, s = task / 20, T = (task / 4) % 5, cq = task & 3;
                asm volatile("ds_write_b64 %0, %1" ::"v"(trd_dst + s * E_COPY + (4 * cq) * E_COL + T * 8), "v"(tv[i]) : "memory");
                if (s == 0) {      // copy 0 spans dY rows -2 .. 17: every element of the tile once (the rest are zeros)
                    accb += __uint_as_float(tv[i].x << 16);
                    accb += __uint_as_float(tv[i].x & 0xffff0000u);
                    accb += __uint_as_float(tv[i].y << 16);
                    accb += __uint_as_float(tv[i].y & 0xffff0000u);
                }
            }
        }
        DWM_BARRIER();      // planar images complete; the raw tiles are dead

        if (tile + 1 < t_end) issue_dma(tile + 1);      // streams in under the products (every LDS access below is assembly: no vmcnt wait)

        // ---- products ----
        wgm_column<0>(a_base, b_base, acc);
        wgm_column<1>(a_base, b_base, acc);
        wgm_column<2>(a_base, b_base, acc);
        wgm_column<3>(a_base, b_base, acc);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- wavefronts -> workgroup: every cell written once, summed in a fixed order ----
    float* red = reinterpret_cast<float*>(smem_wgm);      // [WAVES][NT - 1][CH] taps, then [WAVES][4][CH] bias shares
    float* redb = red + WAVES * (NT - 1) * CH;
#pragma unroll
    for (int kyg = 0; kyg < 2; ++kyg)
#pragma unroll
        for (int kxg = 0; kxg < 2; ++kxg)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int ky = 4 * kyg + mn, kx = 4 * kxg + m;
                if (ky < KS && kx < KS) red[(wid * (NT - 1) + ky * KS + kx) * CH + chl] = acc[kyg][kxg][m];
            }
    redb[(wid * 4 + tg) * CH + ti] = accb;
    __syncthreads();
    float* out = partials + (int64_t)blockIdx.x * NT * C;
    for (int i = tid; i < NT * CH; i += 64 * WAVES) {
        const int tap = i / CH, c = i % CH;
        float s = 0.f;
        if (tap < NT - 1) {
            for (int w = 0; w < WAVES; ++w) s += red[(w * (NT - 1) + tap) * CH + c];
        } else {
            for (int w = 0; w < WAVES * 4; ++w) s += redb[w * CH + c];
        }
        out[(int64_t)tap * C + c0 + c] = s;
    }
}

}  // namespace

// Workgroups per channel slab (== partial rows of the workspace) the kernel is launched with; 0: shape not eligible.
int iseg_dwconv7_wgrad_mfma_blocks(int N, int H, int W, int C, int K, int dil) {
    if (K != KS || dil != 1 || C % 32 != 0 || N <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t ntiles = (int64_t)N * ((H + TR - 1) / TR) * ((W + TC - 1) / TC);
    if (ntiles >= (1ll << 30)) return 0;
    // two resident workgroups per CU: ~512 in flight; every workgroup of a slab walks the same number of tiles (+-1)
    int64_t cap = 512 / (C / CH);
    if (cap < 8) cap = 8;
    const int64_t rounds = ceil_div64(ntiles, cap);
    int64_t bx = ceil_div64(ntiles, rounds);
    if (bx % 8 && (bx + 7) / 8 * 8 <= ntiles) bx = (bx + 7) / 8 * 8;
    return (int)bx;
}

// partials: [blocks][K K + 1][C] fp32 (the layout of dwconv_bwd_weight_dma_kernel: 49 taps, then the bias gradient)
bool iseg_dwconv7_wgrad_mfma_launch(const void* x, const void* dy, float* partials, int N, int H, int W, int C, int pad_t, int pad_l, int blocks,
                                    hipStream_t s) {
    if (blocks <= 0 || (((uintptr_t)x | (uintptr_t)dy) & 15) != 0) return false;
    static const bool raised = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&dwconv7_wgrad_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) ==
               hipSuccess;
    }();
    if (!raised) return false;
    const int tiles_h = (H + TR - 1) / TR, tiles_w = (W + TC - 1) / TC;
    const int64_t ntiles = (int64_t)N * tiles_h * tiles_w;
    const int per = (int)ceil_div64(ntiles, blocks);
    hipLaunchKernelGGL(dwconv7_wgrad_mfma_kernel, dim3((unsigned)blocks, C / CH), dim3(64 * WAVES), LDS_BYTES, s, (const bf16_t*)x, (const bf16_t*)dy,
                       partials, N, H, W, C, pad_t, pad_l, tiles_h, tiles_w, per);
    return true;
}

extern "C" int iseg_dwconv2d7_bwd_weight_mfma(const void* x, const void* dy, float* dw, float* db, int accumulate, int N, int H, int W, int C,
                                              int pad_t, int pad_l, void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && dy && dw && N > 0 && H > 0 && W > 0, "iseg_dwconv2d7_bwd_weight_mfma: bad arguments");
    ISEG_REQUIRE((int64_t)N * H * W * C < (1ll << 31), "iseg_dwconv2d7_bwd_weight_mfma: more than 2^31 elements");
    const int blocks = iseg_dwconv7_wgrad_mfma_blocks(N, H, W, C, KS, 1);
    size_t need = (size_t)blocks * NT * C * sizeof(float);
    const size_t promised = iseg_dwconv2d_bwd_weight_workspace_bytes(N, H, W, C, KS);      // (what the header tells the caller to ask for)
    if (promised > need) need = promised;
    if (blocks > 0) ISEG_NEED_WORKSPACE("iseg_dwconv2d7_bwd_weight_mfma", ws, ws_bytes, need);
    if (!iseg_dwconv7_wgrad_mfma_launch(x, dy, (float*)ws, N, H, W, C, pad_t, pad_l, blocks, stream)) {
        iseg_set_error("iseg_dwconv2d7_bwd_weight_mfma: needs bf16 storage, C %% 32 == 0 (C = %d) and 16-byte aligned tensors", C);
        return ISEG_ERR_UNSUPPORTED;
    }
    const int n = NT * C;
    launch_reduce_rows({.partials = (const float*)ws, .P = blocks, .pstride = n, .n = n, .out0 = dw, .out1 = db, .n0 = (int64_t)(NT - 1) * C,
                        .accumulate = accumulate}, stream);
    return iseg_check_launch("iseg_dwconv2d7_bwd_weight_mfma");
}
