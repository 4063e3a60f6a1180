// Implicit-GEMM convolution on the matrix cores (gfx950), bf16 storage, fp32 accumulate.
//
// Replaces keras.layers.Conv2D(padding="same", strides, dilation_rate, groups) wherever the reference builds one with a kernel
// larger than 1x1 or a stride (layers/model_builder.py:54-64 ConvNormAct.conv, layers/aspp.py:41-52 the three dilated 3x3 branches,
// backbones/resnet_blocks.py:175-205 the bottleneck 3x3, backbones/convnext.py:72-75,255-257 the 2x2/s2 (or dilated) downsample,
// layers/simpledecoder.py:21-36) together with both gradients.  No [pixels, kh*kw*Cin] column buffer exists: the K-slices of the
// patch matrix are gathered straight from the NHWC activation while the operand tile is staged (16-byte chunks = 8 channels of one
// tap; taps that fall into TF's "same" halo, and rows / reduction indices past the problem, are zero chunks), and the data gradient
// is the same gather over dy instead of a col2im scatter -- so all three passes are deterministic.
//
//   pass 0  forward       y[m, co]        = sum_{i,j,c}  x[n, oh*sh + i*dh - pt, ow*sw + j*dw - pl, c] * w[i,j,c,co]      m = (n,oh,ow)
//   pass 1  data grad     dx[m', c]       = sum_{i,j,co} dy[n, (h + pt - i*dh)/sh, (w + pl - j*dw)/sw, co] * w[i,j,c,co]   m' = (n,h,w)
//                                           (a tap contributes only where both quotients are exact and inside the output map)
//   pass 2  weight grad   dw[(i,j,c), co] = sum_m        x[n, oh*sh + i*dh - pt, ow*sw + j*dw - pl, c] * dy[m, co]
//   pass 3  data grad of a STRIDED convolution (dilation 1), by stride phase: the input pixels with h = a (mod sh), w = b (mod sw) only ever
//           meet the taps i = (a + pt) mod sh + t*sh, j = (b + pl) mod sw + u*sw, and for those (h + pt - i) / sh = hq + (a + pt) / sh - t is
//           exact -- so each of the sh*sw phases is a stride-1 gather over dy with its own (smaller) tap grid: no zero products on the matrix
//           cores (the plain gather form of pass 1 multiplies 1 - 1/(sh*sw) zeros), no column buffer, no col2im pass.  All phases run in one
//           launch (blockIdx.y); the epilogue scatters a phase's rows to their pixels of dx.
//
// Each pass is the register-staged MFMA main loop of gemm_impl.h (128 x BN tile, 8 wavefronts, v_mfma_f32_16x16x32_bf16, LDS
// fragments by ds_read_b128 / ds_read_b64_tr_b16, per-wave epilogue slab) with the A stager replaced by a gather: the row part of
// every chunk address (pixel -> n, oh, ow) is decoded once per workgroup, only the tap (k -> i, j, c) changes per K-tile.
// Split-K over the reduction (deterministic fp32 slabs, same reducer as iseg_gemm) fills the chip for the skinny problems
// (ASPP at 16x16: M = 4096, N = 256, K = 6912; weight gradients: K = pixels).  Groups run as grid.z.
#include <type_traits>

#include "gemm_impl.h"

using namespace iseg_mm;

namespace {

struct ConvP {
    const bf16_t* src;      // gathered tensor: x (pass 0, 2) or dy (pass 1), NHWC
    int Hs, Ws, Cs;         // its spatial size and total channel count (row stride)
    int Hr, Wr;             // the grid the GEMM rows (pass 0, 1) or reduction index (pass 2) runs over: output map (0, 2), input map (1)
    int Cg;                 // channels of one group in the gathered tensor
    int kw;
    int sh, sw, dh, dw, pt, pl;
    int groups;
};

// one stride phase of pass 3
struct PhaseP {
    int Hq, Wq;             // pixels of this phase per image: h = hq * sh + a, w = wq * sw + b
    int a, b;
    int q0h, q0w;           // dy row of tap t: hq + q0h - t
    int Th, Tw;             // tap grid of the phase
    int tap0;               // weight tap of (t, u): tap0 + t * sh * kw + u * sw
    int M, K;               // rows (N * Hq * Wq) and reduction (Th * Tw * Cout_g) of the phase
};
constexpr int MAX_PHASES = 16;
struct PhaseTable {
    PhaseP ph[MAX_PHASES];
    int H, W, sh, sw, kw;
};
struct NoPhases {};

// GEMM row of a phase -> pixel of dx
struct PhaseRows {
    int hw, wq, H, W, sh, sw, a, b;
    __device__ __forceinline__ int64_t operator()(int64_t m) const {
        const int n = (int)(m / hw), rem = (int)(m % hw);
        return ((int64_t)n * H + (rem / wq) * sh + a) * W + (rem % wq) * sw + b;
    }
};

constexpr int INVALID = -(1 << 28);

// Several convolutions of ONE input (stride 1, "same" padding, one group, the same channel counts): what differs from branch to branch.
struct BranchP {
    const bf16_t* src;      // gathered tensor and its row stride in channels: x (pass 0, 2; the same for every branch) or this branch's dy (pass 1)
    const bf16_t* B;        // pass 0: K-contiguous kernel copy [Cout][kh*kw*Cin]; pass 1: Keras kernel; pass 2: this branch's dy
    void* D;                // pass 0: y at its column offset; pass 2: dW (fp32)
    const float* bias;      // pass 0
    int64_t ldb, ldd;
    int Cs;
    int kw, dh, dw, pt, pl;
    int K;                  // pass 0: reduction length kh*kw*Cin; pass 1: END of the branch's range in the joined reduction; pass 2: rows of dW
};
constexpr int MAX_BRANCHES = ISEG_CONV_MAX_BRANCHES;
struct BranchTable {
    BranchP b[MAX_BRANCHES];
    int count;
};
struct NoBranches {};

}  // namespace

#include "conv_igemm_dma.h"

namespace {

// 8 consecutive channels `c` of pixel (nb + ih * Ws + iw) of the gathered tensor, or zeros
__device__ __forceinline__ bf16x8 gather8(const ConvP& p, int nb, int ih, int iw, int c, bool ok) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
    if (ok && ih >= 0 && ih < p.Hs && iw >= 0 && iw < p.Ws) v = *reinterpret_cast<const bf16x8*>(p.src + ((int64_t)(nb + ih * p.Ws + iw)) * p.Cs + c);
    return v;
}

// PASS 0 / 1: K-contiguous A (rows = pixels, k = (tap, channel)); PASS 2: MN-contiguous A (rows = (tap, channel), k = pixel)
template <int ROWS, int NT, int BK, int PASS> struct GatherStager : Stager<ROWS, PASS != 2, NT, BK> {
    using Base = Stager<ROWS, PASS != 2, NT, BK>;
    using G = typename Base::G;
    static constexpr int PT = Base::PER_THREAD;
    int a0[PT], a1[PT], a2[PT];      // row-side decode, fixed for the whole reduction

    // rows: first row of the tile; R: number of valid rows; coff: channel offset of this group in the gathered tensor
    __device__ __forceinline__ void prepare(const ConvP& p, int64_t row0, int64_t R, int coff, int tid) {
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int c = tid + i * NT;
            int r, k;
            Base::decode(c, r, k);
            const int64_t row = row0 + r;
            a0[i] = INVALID;
            a1[i] = a2[i] = 0;
            if ((G::chunks % NT != 0 && c >= G::chunks) || row >= R) continue;
            if (PASS == 0) {            // row = output pixel: top-left tap position and image base
                const int hw = p.Hr * p.Wr, n = (int)(row / hw), rem = (int)(row % hw);
                a0[i] = (rem / p.Wr) * p.sh - p.pt;
                a1[i] = (rem % p.Wr) * p.sw - p.pl;
                a2[i] = n * p.Hs * p.Ws;
            } else if (PASS == 1) {     // row = input pixel: h + pt, w + pl and the image base in dy
                const int hw = p.Hr * p.Wr, n = (int)(row / hw), rem = (int)(row % hw);
                a0[i] = rem / p.Wr + p.pt;
                a1[i] = rem % p.Wr + p.pl;
                a2[i] = n * p.Hs * p.Ws;
            } else {                    // row = (tap, channel): tap offset and channel
                const int ij = (int)(row / p.Cg), ch = (int)(row % p.Cg);
                a0[i] = (ij / p.kw) * p.dh - p.pt;
                a1[i] = (ij % p.kw) * p.dw - p.pl;
                a2[i] = coff + ch;
            }
        }
    }
    __device__ __forceinline__ void gather(const ConvP& p, int64_t k0, int64_t Kend, int coff, int tid) {
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int c = tid + i * NT;
            if (G::chunks % NT == 0 || c < G::chunks) {
                int r, k;
                Base::decode(c, r, k);
                const int kk = (int)(k0 + k);
                const bool ok = a0[i] != INVALID && kk < Kend;
                if (PASS == 0) {
                    const int ij = (int)(kk / p.Cg), ch = (int)(kk % p.Cg);
                    this->regs[i] = gather8(p, a2[i], a0[i] + (ij / p.kw) * p.dh, a1[i] + (ij % p.kw) * p.dw, coff + ch, ok);
                } else if (PASS == 1) {
                    const int ij = (int)(kk / p.Cg), ch = (int)(kk % p.Cg);
                    const int th = a0[i] - (ij / p.kw) * p.dh, tw = a1[i] - (ij % p.kw) * p.dw;
                    const bool hit = ok && th >= 0 && tw >= 0 && th % p.sh == 0 && tw % p.sw == 0;
                    this->regs[i] = gather8(p, a2[i], th / p.sh, tw / p.sw, coff + ch, hit);
                } else {
                    const int hw = p.Hr * p.Wr, n = (int)(kk / hw), rem = (int)(kk % hw);
                    this->regs[i] = gather8(p, n * p.Hs * p.Ws, (rem / p.Wr) * p.sh + a0[i], (rem % p.Wr) * p.sw + a1[i], a2[i], ok);
                }
            }
        }
    }
};

// PASS 1's B operand: B(k = (tap, co), n = c) = w[tap][c][co], i.e. K-contiguous rows of length Cout_g inside each tap's [Cin_g, Cout]
// block.  wg = w + group column offset; tap_stride = Cin_g * Cout; ld = Cout.
template <int ROWS, int NT, int BK> struct TapWeightStager : Stager<ROWS, true, NT, BK> {
    using Base = Stager<ROWS, true, NT, BK>;
    using G = typename Base::G;
    // (tw, tap0, tsh, tsw): reduction tap ij = (t, u) of a tw-wide tap grid reads weight tap tap0 + t * tsh + u * tsw (pass 1: the identity)
    __device__ __forceinline__ void load_taps(const bf16_t* __restrict__ wg, int64_t ld, int64_t tap_stride, int cout_g, int64_t n0, int64_t k0,
                                              int64_t R, int64_t Kend, int tid, int tw, int tap0, int tsh, int tsw) {
#pragma unroll
        for (int i = 0; i < Base::PER_THREAD; ++i) {
            const int c = tid + i * NT;
            if (G::chunks % NT == 0 || c < G::chunks) {
                int r, k;
                Base::decode(c, r, k);
                const int kk = (int)(k0 + k);
                const int64_t row = n0 + r;
                bf16x8 v;
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = (bf16_t)0.f;
                if (row < R && kk < Kend) {
                    const int ij = (int)(kk / cout_g), co = (int)(kk % cout_g);
                    const int tap = tap0 + (ij / tw) * tsh + (ij % tw) * tsw;
                    v = *reinterpret_cast<const bf16x8*>(wg + tap * tap_stride + row * ld + co);
                }
                this->regs[i] = v;
            }
        }
    }
};

// one output tile of a pass; grp = channel group.  RAGGED: the grid is sized for the largest of several problems, a tile past this one's rows leaves
template <int WM, int WN, int FM, int FN, int PASS, int BK, class TO, bool RAGGED = false>
__device__ __forceinline__ void conv_igemm_tile(ConvP p, const bf16_t* __restrict__ Bop, int64_t ldb, int64_t b_group_stride, int64_t tap_stride,
                                                TO* __restrict__ D, int64_t ldd, int64_t d_group_stride, int64_t M, int64_t N, int64_t K, int tiles_n,
                                                int ntiles, int64_t k_per_split, float* __restrict__ slabs, int64_t slab_group_stride, Epi epi,
                                                int vecD, const typename std::conditional<PASS == 3, PhaseTable, NoPhases>::type& phases, int grp) {
    constexpr bool AKC = PASS != 2, BKC = PASS == 1 || PASS == 3;
    constexpr int GPASS = PASS == 3 ? 1 : PASS;      // a phase is a stride-1 data-gradient gather in quotient coordinates
    constexpr int NT = WM * WN * 64;
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    constexpr int TM = FM * 16, TN = FN * 16;
    constexpr int KS = BK / 32;
    using GA = TileGeom<BM, AKC, BK>;
    using GB = TileGeom<BN, BKC, BK>;
    constexpr int STAGE_ELEMS = GA::elems + GB::elems;
    constexpr int EPI_BYTES = WM * WN * 32 * (TN + 4) * 4;
    constexpr int LDS_BYTES = (STAGE_ELEMS * 2 > EPI_BYTES) ? STAGE_ELEMS * 2 : EPI_BYTES;
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    bf16_t* const lds = reinterpret_cast<bf16_t*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int coff = grp * p.Cg;
    Bop += grp * b_group_stride;
    D += grp * d_group_stride;
    if (slabs) slabs += grp * slab_group_stride;
    if (epi.bias) epi.bias += grp * N;

    int t, ksplit;
    int tw = p.kw, tap0 = 0, tsh = p.kw, tsw = 1;
    PhaseRows rows{};
    if constexpr (PASS == 3) {
        const PhaseP& ph = phases.ph[blockIdx.y];
        M = ph.M;
        K = ph.K;
        k_per_split = K;
        t = blockIdx.x;
        ksplit = 0;
        if ((int64_t)(t / tiles_n) * BM >= M) return;      // (workgroup-uniform: the grid is sized for the largest phase)
        p.Hr = ph.Hq, p.Wr = ph.Wq, p.kw = ph.Tw, p.pt = ph.q0h, p.pl = ph.q0w;
        p.sh = p.sw = p.dh = p.dw = 1;
        tw = ph.Tw, tap0 = ph.tap0, tsh = phases.sh * phases.kw, tsw = phases.sw;
        rows = PhaseRows{ph.Hq * ph.Wq, ph.Wq, phases.H, phases.W, phases.sh, phases.sw, ph.a, ph.b};
    } else {
        tile_and_split(ntiles, t, ksplit);
    }
    const int tile_n = t % tiles_n, tile_m = t / tiles_n;
    const int64_t m0 = (int64_t)tile_m * BM, n0 = (int64_t)tile_n * BN;
    if (RAGGED && m0 >= M) return;      // (workgroup-uniform)
    const int64_t kbeg = (int64_t)ksplit * k_per_split;
    const int64_t kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;
    const int nk = (int)((kend - kbeg + BK - 1) / BK);

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    GatherStager<BM, NT, BK, GPASS> sa;
    typename std::conditional<BKC, TapWeightStager<BN, NT, BK>, Stager<BN, false, NT, BK>>::type sb;
    sa.prepare(p, m0, M, coff, tid);

    auto load_b = [&](int64_t k0) {
        if constexpr (BKC) sb.load_taps(Bop, ldb, tap_stride, p.Cg, n0, k0, N, kend, tid, tw, tap0, tsh, tsw);
        else sb.load(Bop, ldb, n0, k0, N, kend, true, tid);
    };

    sa.gather(p, kbeg, kend, coff, tid);
    load_b(kbeg);
    sa.store(lds, tid);
    sb.store(lds + GA::elems, tid);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) {
            const int64_t k0 = kbeg + (int64_t)(kt + 1) * BK;
            sa.gather(p, k0, kend, coff, tid);
            load_b(k0);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 af[FM], bfr[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = read_frag<BM, AKC, BK>(lds, wm * TM + i * 16, ks, lane);
#pragma unroll
            for (int j = 0; j < FN; ++j) bfr[j] = read_frag<BN, BKC, BK>(lds + GA::elems, wn * TN + j * 16, ks, lane);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            sa.store(lds, tid);
            sb.store(lds + GA::elems, tid);
            __syncthreads();
        }
    }
    if constexpr (PASS == 3) tile_epilogue<WM, WN, FM, FN, TO, PhaseRows>(acc, smem, D, ldd, M, N, m0, n0, wm, wn, wid, lane, nullptr, epi, false, vecD, 0, rows);
    else tile_epilogue<WM, WN, FM, FN, TO>(acc, smem, D, ldd, M, N, m0, n0, wm, wn, wid, lane, slabs, epi, false, vecD, ksplit);
}

template <int WM, int WN, int FM, int FN, int PASS, int BK, class TO>
__global__ __launch_bounds__(WM* WN * 64) void conv_igemm_kernel(ConvP p, const bf16_t* __restrict__ Bop, int64_t ldb, int64_t b_group_stride,
                                                                  int64_t tap_stride, TO* __restrict__ D, int64_t ldd, int64_t d_group_stride,
                                                                  int64_t M, int64_t N, int64_t K, int tiles_n, int ntiles,
                                                                  int64_t k_per_split, float* __restrict__ slabs, int64_t slab_group_stride,
                                                                  Epi epi, int vecD,
                                                                  typename std::conditional<PASS == 3, PhaseTable, NoPhases>::type phases) {
    conv_igemm_tile<WM, WN, FM, FN, PASS, BK, TO>(p, Bop, ldb, b_group_stride, tap_stride, D, ldd, d_group_stride, M, N, K, tiles_n, ntiles,
                                                  k_per_split, slabs, slab_group_stride, epi, vecD, phases, blockIdx.z);
}

// The weight gradients of several convolutions of one input: blockIdx.z = branch, each with its own taps (p.kw / dilation / padding), dy and dW.
// grid.x covers the branch with the most taps; one pass over the pixels, no slabs.
template <int WM, int WN, int FM, int FN, int BK>
__global__ __launch_bounds__(WM* WN * 64) void conv_branches_wgrad_kernel(ConvP p, BranchTable tab, int64_t N, int64_t K, int tiles_n, int ntiles,
                                                                           Epi epi, int vecD) {
    const BranchP& br = tab.b[blockIdx.z];
    p.kw = br.kw, p.dh = br.dh, p.dw = br.dw, p.pt = br.pt, p.pl = br.pl;
    conv_igemm_tile<WM, WN, FM, FN, 2, BK, float, true>(p, br.B, br.ldb, 0, 0, (float*)br.D, br.ldd, 0, br.K, N, K, tiles_n, ntiles, K, nullptr, 0, epi,
                                                        vecD, NoPhases{}, 0);
}

struct Problem {
    int64_t M, N, K;            // per group
    ConvP p;
    const bf16_t* B;
    int64_t ldb, b_group_stride, tap_stride;
    void* D;
    int64_t ldd, d_group_stride;
    int out_dtype;
    const float* bias;
    int accumulate;
    int groups;
};

int conv_splits(int64_t M, int64_t N, int64_t K, int groups) {
    const int64_t tiles = ceil_div64(M, 128) * ceil_div64(N, N <= 64 ? 64 : 128) * groups;
    if (tiles >= 256 || K < 1024) return 1;
    int64_t want = 512 / tiles;
    const int64_t maxs = K / 512 > 0 ? K / 512 : 1;
    if (want > maxs) want = maxs;
    return (int)(want < 1 ? 1 : want);
}

// conv_splits' answer for one group, cut at multiples of 64 (the K-tile of every pass), slabs of M x N
SplitPlan conv_plan(int64_t M, int64_t N, int64_t K) { return split_plan(K, conv_splits(M, N, K, 1), 64, M, N); }

// output tiles of the register-staged passes: 128 x 128 (8 wavefronts of 64 x 32), 128 x 64 for narrow outputs
struct T128 { enum { WM = 2, WN = 4, FM = 4, FN = 2 }; };
struct T64 { enum { WM = 4, WN = 2, FM = 2, FN = 2 }; };
template <class F> void with_tile(int64_t N, F&& launch) {
    if (N <= 64) launch(T64{});
    else launch(T128{});
}

template <int PASS, class TO> int run(const Problem& q, void* ws, size_t ws_bytes, hipStream_t stream, const char* what) {
    // grouped layers are small: one pass, no slabs (so split problems have one group)
    const SplitPlan plan = q.groups > 1 ? split_plan(q.K, 1, 64, q.M, q.N) : conv_plan(q.M, q.N, q.K);
    float* slabs = nullptr;
    if (plan.nsplit > 1) {
        ISEG_NEED_WORKSPACE(what, ws, ws_bytes, plan.slab_bytes);
        slabs = (float*)ws;
    }
    const Epi epi = plain_epi(q.bias, q.accumulate);
    const int vecD = ((uintptr_t)q.D % 16 == 0) && (q.ldd % 8 == 0) && (q.d_group_stride % 8 == 0) && (!q.bias || (uintptr_t)q.bias % 16 == 0) &&
                     (q.N % 4 == 0);
    const int64_t slab_group_stride = 0;
    with_tile(q.N, [&](auto tile) {
        constexpr int WM = decltype(tile)::WM, WN = decltype(tile)::WN, FM = decltype(tile)::FM, FN = decltype(tile)::FN;
        constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
        const int tiles_m = (int)ceil_div64(q.M, BM), tiles_n = (int)ceil_div64(q.N, BN);
        hipLaunchKernelGGL((conv_igemm_kernel<WM, WN, FM, FN, PASS, 64, TO>), dim3(tiles_m * tiles_n, plan.eff_split, q.groups), dim3(WM * WN * 64), 0,
                           stream, q.p, q.B, q.ldb, q.b_group_stride, q.tap_stride, (TO*)q.D, q.ldd, q.d_group_stride, q.M, q.N, q.K, tiles_n,
                           tiles_m * tiles_n, plan.kps, slabs, slab_group_stride, epi, vecD, NoPhases{});
    });
    if (!slabs) return iseg_check_launch(what);
    // slab-order sum + epilogue through the GEMM reducer (deterministic)
    return gemm_reduce(epi, q.D, q.ldd, q.out_dtype, q.M, q.N, slabs, plan, stream);
}

// pass 3: every stride phase of a strided data gradient in one launch (grid.y = phase, grid.z = group); phases no tap reaches (kernel
// smaller than the stride) keep the zeros dx is cleared to first
int run_phases(const Problem& q, const iseg_conv_geom* g, hipStream_t stream, const char* what) {
    PhaseTable tab{};
    tab.H = g->H, tab.W = g->W, tab.sh = g->sh, tab.sw = g->sw, tab.kw = g->KW;
    const int og = g->Cout / g->groups;
    int count = 0;
    int64_t maxM = 0;
    bool holes = false;
    for (int a = 0; a < g->sh; ++a)
        for (int b = 0; b < g->sw; ++b) {
            const int Hq = a < g->H ? (g->H - a + g->sh - 1) / g->sh : 0, Wq = b < g->W ? (g->W - b + g->sw - 1) / g->sw : 0;
            if (Hq == 0 || Wq == 0) continue;
            const int rh = (a + g->pt) % g->sh, rw = (b + g->pl) % g->sw;
            const int Th = rh < g->KH ? (g->KH - rh + g->sh - 1) / g->sh : 0, Tw = rw < g->KW ? (g->KW - rw + g->sw - 1) / g->sw : 0;
            if (Th == 0 || Tw == 0) {
                holes = true;
                continue;
            }
            PhaseP& ph = tab.ph[count++];
            ph.Hq = Hq, ph.Wq = Wq, ph.a = a, ph.b = b;
            ph.q0h = (a + g->pt) / g->sh, ph.q0w = (b + g->pl) / g->sw;
            ph.Th = Th, ph.Tw = Tw;
            ph.tap0 = rh * g->KW + rw;
            ph.M = (int)((int64_t)g->N * Hq * Wq);
            ph.K = Th * Tw * og;
            if (ph.M > maxM) maxM = ph.M;
        }
    if (holes) {
        const hipError_t e = hipMemsetAsync(q.D, 0, (size_t)g->N * g->H * g->W * g->Cin * sizeof(bf16_t), stream);
        if (e != hipSuccess) {
            iseg_set_error("%s: clearing dx failed: %s", what, hipGetErrorString(e));
            return ISEG_ERR_HIP;
        }
    }
    if (count == 0) return ISEG_OK;
    const Epi epi = plain_epi(nullptr, 0);
    const int vecD = ((uintptr_t)q.D % 16 == 0) && (q.ldd % 8 == 0) && (q.d_group_stride % 8 == 0) && (q.N % 4 == 0);
    with_tile(q.N, [&](auto tile) {
        constexpr int WM = decltype(tile)::WM, WN = decltype(tile)::WN, FM = decltype(tile)::FM, FN = decltype(tile)::FN;
        constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
        const int tiles_m = (int)ceil_div64(maxM, BM), tiles_n = (int)ceil_div64(q.N, BN);
        hipLaunchKernelGGL((conv_igemm_kernel<WM, WN, FM, FN, 3, 64, bf16_t>), dim3(tiles_m * tiles_n, count, q.groups), dim3(WM * WN * 64), 0, stream,
                           q.p, q.B, q.ldb, q.b_group_stride, q.tap_stride, (bf16_t*)q.D, q.ldd, q.d_group_stride, maxM, q.N, (int64_t)0, tiles_n,
                           tiles_m * tiles_n, (int64_t)0, (float*)nullptr, (int64_t)0, epi, vecD, tab);
    });
    return iseg_check_launch(what);
}

// ---- LDS-DMA form (conv_igemm_dma.h): forward on the K-contiguous kernel copy, stride-1 data gradient on the Keras kernel ----
bool dma_conv_eligible(const Problem& q, const iseg_conv_geom* g, int pass) {
    if (g->groups != 1 || q.p.Cg % 64 != 0 || q.N % 8 != 0 || q.N < 64 || q.M < 64 || q.K < 128) return false;
    if (pass == 1 && (g->sh != 1 || g->sw != 1)) return false;      // strided data gradients run by stride phase (pass 3)
    if (((uintptr_t)q.p.src | (uintptr_t)q.B | (uintptr_t)q.D) % 16 || q.ldd % 8 || q.ldb % 8 || q.p.Cs % 8) return false;
    if (q.bias && (uintptr_t)q.bias % 16) return false;
    return true;
}

template <int PASS> int run_dma(const Problem& q, void* ws, size_t ws_bytes, hipStream_t stream, const char* what) {
    const SplitPlan plan = conv_plan(q.M, q.N, q.K);
    float* slabs = nullptr;
    if (plan.nsplit > 1) {
        ISEG_NEED_WORKSPACE(what, ws, ws_bytes, plan.slab_bytes);
        slabs = (float*)ws;
    }
    const Epi epi = plain_epi(q.bias, q.accumulate);
    auto launch = [&](auto tile) {
        constexpr int WM = decltype(tile)::WM, WN = decltype(tile)::WN, NS = decltype(tile)::NS;
        constexpr int BM = WM * 64, BN = WN * 64;
        constexpr int lds = NS * (BM + BN) * 128;
        const int tiles_m = (int)ceil_div64(q.M, BM), tiles_n = (int)ceil_div64(q.N, BN);
        static const bool raised = [] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_igemm_dma_kernel<WM, WN, NS, PASS, bf16_t>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        }();
        (void)raised;
        hipLaunchKernelGGL((conv_igemm_dma_kernel<WM, WN, NS, PASS, bf16_t>), dim3(tiles_m * tiles_n, plan.eff_split, 1), dim3(WM * WN * 64), lds, stream,
                           q.p, q.B, q.ldb, q.tap_stride, (bf16_t*)q.D, q.ldd, q.M, q.N, q.K, tiles_n, tiles_m * tiles_n, plan.kps, slabs, epi);
    };
    struct D256 { enum { WM = 4, WN = 2, NS = 3 }; };      // the LDS-DMA kernel's tiles: 256 x 128 with three stages, 128 x 128 with two
    struct D128 { enum { WM = 2, WN = 2, NS = 2 }; };
    if (ceil_div64(q.M, 256) * ceil_div64(q.N, 128) * plan.eff_split >= 192) launch(D256{});
    else launch(D128{});
    if (!slabs) return iseg_check_launch(what);
    return gemm_reduce(epi, q.D, q.ldd, q.out_dtype, q.M, q.N, slabs, plan, stream);
}

bool geom_ok(const iseg_conv_geom* g) {
    return g && g->N > 0 && g->H > 0 && g->W > 0 && g->Cin > 0 && g->Cout > 0 && g->KH > 0 && g->KW > 0 && g->sh > 0 && g->sw > 0 && g->dh > 0 &&
           g->dw > 0 && g->Ho > 0 && g->Wo > 0 && g->groups > 0 && g->Cin % g->groups == 0 && g->Cout % g->groups == 0;
}

}  // namespace

extern "C" int iseg_conv2d_igemm_supported(const iseg_conv_geom* g, int dtype) {
    if (!geom_ok(g) || dtype != ISEG_BF16) return 0;
    const int cg = g->Cin / g->groups, og = g->Cout / g->groups;
    // 16-byte gathers: 8 channels of one tap per chunk on both the x side and the dy side; split-K over groups is not wired (the
    // grouped layers of the reference are small), so grouped problems must fit one pass
    if (cg % 8 != 0 || og % 8 != 0) return 0;
    if ((int64_t)g->N * g->H * g->W >= (1ll << 31) / 8 || (int64_t)g->N * g->Ho * g->Wo >= (1ll << 31) / 8) return 0;
    return 1;
}

namespace iseg_mm {
size_t conv_patch_wgrad_workspace(const iseg_conv_geom* g);      // conv_patchify.hip
}

extern "C" size_t iseg_conv2d_igemm_workspace_bytes(const iseg_conv_geom* g, int pass) {
    if (!geom_ok(g) || g->groups > 1) return 0;
    if (pass == 3) return iseg_mm::conv_patch_wgrad_workspace(g);
    const int64_t Mo = (int64_t)g->N * g->Ho * g->Wo, Mi = (int64_t)g->N * g->H * g->W, Kd = (int64_t)g->KH * g->KW * g->Cin;
    int64_t M, N, K;
    if (pass == 0) M = Mo, N = g->Cout, K = Kd;
    else if (pass == 1) M = Mi, N = g->Cin, K = (int64_t)g->KH * g->KW * g->Cout;
    else M = Kd, N = g->Cout, K = Mo;
    return conv_plan(M, N, K).slab_bytes;
}

#define CONV_COMMON(name)                                                                                                             \
    ISEG_REQUIRE(geom_ok(g), name ": bad geometry");                                                                                 \
    ISEG_REQUIRE(iseg_conv2d_igemm_supported(g, dtype), name ": needs bf16 storage and channels per group that are multiples of 8 " \
                                                              "(Cin %d, Cout %d, groups %d, dtype %d)", g->Cin, g->Cout, g->groups, dtype); \
    const int cg = g->Cin / g->groups, og = g->Cout / g->groups;                                                                     \
    (void)cg;                                                                                                                         \
    (void)og

extern "C" int iseg_conv2d_igemm_fwd(const void* x, const void* w, const float* bias, void* y, const iseg_conv_geom* g, int dtype, void* ws,
                                     size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && w && y, "iseg_conv2d_igemm_fwd: null operand");
    CONV_COMMON("iseg_conv2d_igemm_fwd");
    ISEG_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) == 0, "iseg_conv2d_igemm_fwd: operands must be 16-byte aligned");
    Problem q{};
    q.M = (int64_t)g->N * g->Ho * g->Wo;
    q.N = og;
    q.K = (int64_t)g->KH * g->KW * cg;
    q.p = ConvP{(const bf16_t*)x, g->H, g->W, g->Cin, g->Ho, g->Wo, cg, g->KW, g->sh, g->sw, g->dh, g->dw, g->pt, g->pl, g->groups};
    q.B = (const bf16_t*)w;
    q.ldb = g->Cout;
    q.b_group_stride = og;
    q.D = y;
    q.ldd = g->Cout;
    q.d_group_stride = og;
    q.out_dtype = ISEG_BF16;
    q.bias = bias;
    q.groups = g->groups;
    return run<0, bf16_t>(q, ws, ws_bytes, stream, "iseg_conv2d_igemm_fwd");
}

extern "C" int iseg_conv2d_igemm_fwd_kt(const void* x, const void* wt, const float* bias, void* y, const iseg_conv_geom* g, int dtype, void* ws,
                                        size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && wt && y, "iseg_conv2d_igemm_fwd_kt: null operand");
    CONV_COMMON("iseg_conv2d_igemm_fwd_kt");
    Problem q{};
    q.M = (int64_t)g->N * g->Ho * g->Wo;
    q.N = og;
    q.K = (int64_t)g->KH * g->KW * cg;
    q.p = ConvP{(const bf16_t*)x, g->H, g->W, g->Cin, g->Ho, g->Wo, cg, g->KW, g->sh, g->sw, g->dh, g->dw, g->pt, g->pl, g->groups};
    q.B = (const bf16_t*)wt;
    q.ldb = q.K;
    q.D = y;
    q.ldd = g->Cout;
    q.out_dtype = ISEG_BF16;
    q.bias = bias;
    q.groups = g->groups;
    if (!dma_conv_eligible(q, g, 0)) {
        iseg_set_error("iseg_conv2d_igemm_fwd_kt: one group, Cin %% 64 == 0, Cout %% 8 == 0 and >= 64, 16-byte aligned operands (Cin %d, Cout %d, groups %d)",
                       g->Cin, g->Cout, g->groups);
        return ISEG_ERR_UNSUPPORTED;
    }
    return run_dma<0>(q, ws, ws_bytes, stream, "iseg_conv2d_igemm_fwd_kt");
}

extern "C" int iseg_conv2d_igemm_fwd_kt_supported(const iseg_conv_geom* g, int dtype) {
    if (!geom_ok(g) || dtype != ISEG_BF16) return 0;
    return g->groups == 1 && g->Cin % 64 == 0 && g->Cout % 8 == 0 && g->Cout >= 64 && (int64_t)g->N * g->Ho * g->Wo >= 64 &&
           (int64_t)g->KH * g->KW * g->Cin >= 128;
}

extern "C" int iseg_conv2d_igemm_bwd_data(const void* dy, const void* w, void* dx, const iseg_conv_geom* g, int dtype, void* ws, size_t ws_bytes,
                                          hipStream_t stream) {
    ISEG_REQUIRE(dy && w && dx, "iseg_conv2d_igemm_bwd_data: null operand");
    CONV_COMMON("iseg_conv2d_igemm_bwd_data");
    ISEG_REQUIRE((((uintptr_t)dy | (uintptr_t)w | (uintptr_t)dx) & 15) == 0, "iseg_conv2d_igemm_bwd_data: operands must be 16-byte aligned");
    Problem q{};
    q.M = (int64_t)g->N * g->H * g->W;
    q.N = cg;
    q.K = (int64_t)g->KH * g->KW * og;
    q.p = ConvP{(const bf16_t*)dy, g->Ho, g->Wo, g->Cout, g->H, g->W, og, g->KW, g->sh, g->sw, g->dh, g->dw, g->pt, g->pl, g->groups};
    q.B = (const bf16_t*)w;
    q.ldb = g->Cout;
    q.b_group_stride = og;
    q.tap_stride = (int64_t)cg * g->Cout;
    q.D = dx;
    q.ldd = g->Cin;
    q.d_group_stride = cg;
    q.out_dtype = ISEG_BF16;
    q.groups = g->groups;
    // strided, undilated: one stride-1 gather per stride phase (pass 3) instead of the gather form that multiplies the zeros between the hits
    if ((g->sh > 1 || g->sw > 1) && g->dh == 1 && g->dw == 1 && g->sh * g->sw <= MAX_PHASES)
        return run_phases(q, g, stream, "iseg_conv2d_igemm_bwd_data");
    if (dma_conv_eligible(q, g, 1)) return run_dma<1>(q, ws, ws_bytes, stream, "iseg_conv2d_igemm_bwd_data");
    return run<1, bf16_t>(q, ws, ws_bytes, stream, "iseg_conv2d_igemm_bwd_data");
}

extern "C" int iseg_conv2d_igemm_bwd_weight(const void* x, const void* dy, float* dw, int accumulate, const iseg_conv_geom* g, int dtype, void* ws,
                                            size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && dy && dw, "iseg_conv2d_igemm_bwd_weight: null operand");
    CONV_COMMON("iseg_conv2d_igemm_bwd_weight");
    ISEG_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dw) & 15) == 0, "iseg_conv2d_igemm_bwd_weight: operands must be 16-byte aligned");
    Problem q{};
    q.M = (int64_t)g->KH * g->KW * cg;
    q.N = og;
    q.K = (int64_t)g->N * g->Ho * g->Wo;
    q.p = ConvP{(const bf16_t*)x, g->H, g->W, g->Cin, g->Ho, g->Wo, cg, g->KW, g->sh, g->sw, g->dh, g->dw, g->pt, g->pl, g->groups};
    q.B = (const bf16_t*)dy;
    q.ldb = g->Cout;
    q.b_group_stride = og;
    q.D = dw;
    q.ldd = g->Cout;
    q.d_group_stride = og;
    q.out_dtype = ISEG_F32;
    q.accumulate = accumulate;
    q.groups = g->groups;
    return run<2, float>(q, ws, ws_bytes, stream, "iseg_conv2d_igemm_bwd_weight");
}

// ---- several convolutions of one input (ASPP's pixel-level branches): grouped forward / weight gradient, K-joined data gradient ----
namespace {

bool branches_ok(const iseg_conv_branches* t) {
    if (!t || t->count < 1 || t->count > MAX_BRANCHES || t->N <= 0 || t->H <= 0 || t->W <= 0 || t->Cin <= 0 || t->Cout <= 0) return false;
    for (int i = 0; i < t->count; ++i) {
        const iseg_conv_branch& b = t->b[i];
        if (b.KH <= 0 || b.KW <= 0 || b.dh <= 0 || b.dw <= 0 || b.pt < 0 || b.pl < 0) return false;
    }
    return true;
}

// what the branches share; `src` / `Cs` are the gathered tensor of passes 0 and 2 (the table brings pass 1's)
ConvP branches_shared(const iseg_conv_branches* t, const void* src, int Cs, int Cg) {
    return ConvP{(const bf16_t*)src, t->H, t->W, Cs, t->H, t->W, Cg, 1, 1, 1, 1, 1, 0, 0, 1};
}

template <int PASS, class Tile>
void launch_branches_dma(Tile, const ConvP& p, const BranchTable& tab, int64_t ldb, int64_t tap_stride, bf16_t* D, int64_t ldd, int64_t M, int64_t N,
                         int64_t K, int eff, int64_t kps, float* slabs, const Epi& epi, hipStream_t stream) {
    constexpr int WM = Tile::WM, WN = Tile::WN, FN = Tile::FN, NS = Tile::NS;
    constexpr int BM = WM * 64, BN = WN * FN * 16;
    constexpr int lds = NS * (BM + BN) * 128;
    const int tiles_m = (int)ceil_div64(M, BM), tiles_n = (int)ceil_div64(N, BN);
    static const bool raised = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_branches_dma_kernel<WM, WN, FN, NS, PASS>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
    }();
    (void)raised;
    hipLaunchKernelGGL((conv_branches_dma_kernel<WM, WN, FN, NS, PASS>), dim3(tiles_m * tiles_n, eff, PASS == 0 ? tab.count : 1), dim3(WM * WN * 64), lds,
                       stream, p, tab, ldb, tap_stride, D, ldd, M, N, K, tiles_n, tiles_m * tiles_n, kps, slabs, epi);
}
struct BT256 { enum { WM = 4, WN = 2, FN = 4, NS = 3 }; };
// 128 x 128 as 8 wavefronts of 64 x 32: the grouped forward is ONE workgroup per CU (4 branches x 64 tiles at the flagship), and two wavefronts
// per SIMD hide each other's LDS reads -- 100 us against 115 us for conv_igemm_dma_kernel's 4 wavefronts of 64 x 64 (3 / 4 stages: 97 / 94 us;
// 256 x 128 tiles, half the CUs: 131 us; the four per-branch launches with their reducers: 136 us)
struct BT128 { enum { WM = 2, WN = 4, FN = 2, NS = 2 }; };

}  // namespace

extern "C" int iseg_conv2d_branches_supported(const iseg_conv_branches* t, int dtype) {
    if (!branches_ok(t) || dtype != ISEG_BF16) return 0;
    // the LDS-DMA pipeline's K-step is 64 channels of one tap, on the x side (forward) and on the dy side (data gradient)
    if (t->Cin % 64 != 0 || t->Cout % 64 != 0) return 0;
    const int64_t M = (int64_t)t->N * t->H * t->W;
    return M >= 64 && M < (1ll << 31) / 8;
}

#define BRANCHES_COMMON(name)                                                                                                                  \
    ISEG_REQUIRE(t, name ": null branch table");                                                                                              \
    ISEG_REQUIRE(t->count >= 1 && t->count <= MAX_BRANCHES, name ": %d branches, the table holds 1 .. %d", t->count, MAX_BRANCHES);          \
    ISEG_REQUIRE(branches_ok(t), name ": bad geometry");                                                                                      \
    if (!iseg_conv2d_branches_supported(t, dtype)) {                                                                                          \
        iseg_set_error(name ": needs bf16 storage, Cin and Cout multiples of 64 and at least 64 pixels (Cin %d, Cout %d, dtype %d)", t->Cin,  \
                       t->Cout, dtype);                                                                                                       \
        return ISEG_ERR_UNSUPPORTED;                                                                                                          \
    }                                                                                                                                         \
    const int64_t M = (int64_t)t->N * t->H * t->W

extern "C" int iseg_conv2d_branches_fwd(const void* x, const iseg_conv_branches* t, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    BRANCHES_COMMON("iseg_conv2d_branches_fwd");
    (void)ws;
    (void)ws_bytes;
    ISEG_REQUIRE(x && ((uintptr_t)x & 15) == 0, "iseg_conv2d_branches_fwd: x must be a 16-byte aligned device pointer");
    BranchTable tab{};
    tab.count = t->count;
    for (int i = 0; i < t->count; ++i) {
        const iseg_conv_branch& b = t->b[i];
        ISEG_REQUIRE(b.wt && b.y, "iseg_conv2d_branches_fwd: branch %d: null operand", i);
        bf16_t* const y = (bf16_t*)b.y + b.y_col;
        ISEG_REQUIRE((((uintptr_t)b.wt | (uintptr_t)y | (uintptr_t)b.bias) & 15) == 0 && b.ldy % 8 == 0 && b.y_col >= 0 && b.y_col + t->Cout <= b.ldy,
                     "iseg_conv2d_branches_fwd: branch %d: operands must be 16-byte aligned, the column slice inside a row of ldy %% 8 == 0", i);
        BranchP& d = tab.b[i];
        d.B = (const bf16_t*)b.wt;
        d.K = b.KH * b.KW * t->Cin;
        d.ldb = d.K;
        d.D = y;
        d.ldd = b.ldy;
        d.bias = b.bias;
        d.kw = b.KW, d.dh = b.dh, d.dw = b.dw, d.pt = b.pt, d.pl = b.pl;
    }
    const ConvP p = branches_shared(t, x, t->Cin, t->Cin);
    launch_branches_dma<0>(BT128{}, p, tab, 0, 0, nullptr, 0, M, t->Cout, 0, 1, 0, nullptr, plain_epi(nullptr, 0), stream);
    return iseg_check_launch("iseg_conv2d_branches_fwd");
}

extern "C" int iseg_conv2d_branches_bwd_data(const iseg_conv_branches* t, void* dx, const void* residual, int64_t ldr, int dtype, void* ws,
                                             size_t ws_bytes, hipStream_t stream) {
    BRANCHES_COMMON("iseg_conv2d_branches_bwd_data");
    ISEG_REQUIRE(dx && ((uintptr_t)dx & 15) == 0, "iseg_conv2d_branches_bwd_data: dx must be a 16-byte aligned device pointer");
    ISEG_REQUIRE(!residual || (((uintptr_t)residual & 15) == 0 && ldr % 8 == 0 && ldr >= t->Cin),
                 "iseg_conv2d_branches_bwd_data: the residual must be 16-byte aligned with ldr %% 8 == 0");
    BranchTable tab{};
    tab.count = t->count;
    int64_t K = 0;
    for (int i = 0; i < t->count; ++i) {
        const iseg_conv_branch& b = t->b[i];
        ISEG_REQUIRE(b.dy && b.w, "iseg_conv2d_branches_bwd_data: branch %d: null operand", i);
        ISEG_REQUIRE((((uintptr_t)b.dy | (uintptr_t)b.w) & 15) == 0 && b.lddy % 8 == 0 && b.lddy >= t->Cout && b.lddy < (1ll << 31),
                     "iseg_conv2d_branches_bwd_data: branch %d: operands must be 16-byte aligned, lddy %% 8 == 0", i);
        K += (int64_t)b.KH * b.KW * t->Cout;
        BranchP& d = tab.b[i];
        d.src = (const bf16_t*)b.dy;
        d.Cs = (int)b.lddy;
        d.B = (const bf16_t*)b.w;
        d.K = (int)K;
        d.kw = b.KW, d.dh = b.dh, d.dw = b.dw, d.pt = b.pt, d.pl = b.pl;
    }
    const int64_t N = t->Cin;
    // The K-joined data gradient IS one stride-1 data gradient whose taps are the taps of every branch in a row: it takes that problem's plan, and
    // the caller sizes the slabs by iseg_conv2d_igemm_workspace_bytes (pass 1) of that geometry, a 1 x (all taps) kernel over the same maps.
    // Its tile (256 x 128 from 256 pixels on), flagship (M = 4096, N = 768, K = 7168), kernel only: 256 x 128 tiles, 2 splits + reducer 126 us; 128 x 128 tiles, 2 splits + reducer
    // 132 us; 128 x 128, no split (192 workgroups for 256 CUs) 138 us; 256 x 128, no split 207 us.
    const SplitPlan plan = conv_plan(M, N, K);
    float* slabs = nullptr;
    if (plan.nsplit > 1) {
        ISEG_NEED_WORKSPACE("iseg_conv2d_branches_bwd_data", ws, ws_bytes, plan.slab_bytes);
        slabs = (float*)ws;
    }
    Epi epi = plain_epi(nullptr, 0);
    epi.residual = residual, epi.ldr = ldr;
    const ConvP p = branches_shared(t, nullptr, 0, t->Cout);
    const int64_t tap_stride = (int64_t)t->Cin * t->Cout;
    if (M >= 256) launch_branches_dma<1>(BT256{}, p, tab, t->Cout, tap_stride, (bf16_t*)dx, N, M, N, K, plan.eff_split, plan.kps, slabs, epi, stream);
    else launch_branches_dma<1>(BT128{}, p, tab, t->Cout, tap_stride, (bf16_t*)dx, N, M, N, K, plan.eff_split, plan.kps, slabs, epi, stream);
    if (!slabs) return iseg_check_launch("iseg_conv2d_branches_bwd_data");
    return gemm_reduce(epi, dx, N, ISEG_BF16, M, N, slabs, plan, stream);
}

extern "C" int iseg_conv2d_branches_bwd_weight(const void* x, const iseg_conv_branches* t, int accumulate, int dtype, void* ws, size_t ws_bytes,
                                               hipStream_t stream) {
    BRANCHES_COMMON("iseg_conv2d_branches_bwd_weight");
    (void)ws;
    (void)ws_bytes;
    ISEG_REQUIRE(x && ((uintptr_t)x & 15) == 0, "iseg_conv2d_branches_bwd_weight: x must be a 16-byte aligned device pointer");
    BranchTable tab{};
    tab.count = t->count;
    int maxK = 0;
    for (int i = 0; i < t->count; ++i) {
        const iseg_conv_branch& b = t->b[i];
        ISEG_REQUIRE(b.dy && b.gw, "iseg_conv2d_branches_bwd_weight: branch %d: null operand", i);
        ISEG_REQUIRE((((uintptr_t)b.dy | (uintptr_t)b.gw) & 15) == 0 && b.lddy % 8 == 0 && b.lddy >= t->Cout,
                     "iseg_conv2d_branches_bwd_weight: branch %d: operands must be 16-byte aligned, lddy %% 8 == 0", i);
        BranchP& d = tab.b[i];
        d.B = (const bf16_t*)b.dy;
        d.ldb = b.lddy;
        d.D = b.gw;
        d.ldd = t->Cout;
        d.K = b.KH * b.KW * t->Cin;
        d.kw = b.KW, d.dh = b.dh, d.dw = b.dw, d.pt = b.pt, d.pl = b.pl;
        if (d.K > maxK) maxK = d.K;
    }
    const Epi epi = plain_epi(nullptr, accumulate);
    const ConvP p = branches_shared(t, x, t->Cin, t->Cin);
    const int64_t N = t->Cout;
    with_tile(N, [&](auto tile) {
        constexpr int WM = decltype(tile)::WM, WN = decltype(tile)::WN, FM = decltype(tile)::FM, FN = decltype(tile)::FN;
        constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
        const int tiles_m = (int)ceil_div64(maxK, BM), tiles_n = (int)ceil_div64(N, BN);
        hipLaunchKernelGGL((conv_branches_wgrad_kernel<WM, WN, FM, FN, 64>), dim3(tiles_m * tiles_n, 1, tab.count), dim3(WM * WN * 64), 0, stream, p, tab,
                           N, M, tiles_n, tiles_m * tiles_n, epi, 1);
    });
    return iseg_check_launch("iseg_conv2d_branches_bwd_weight");
}
