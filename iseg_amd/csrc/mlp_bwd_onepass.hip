// Backward pass of the fused ConvNeXt MLP at C = 96 in ONE pass over the rows (backbones/convnext.py:51-63 of the reference, with the
// LayerNorm of :52 on the row load): data gradient through the LayerNorm AND every parameter gradient, the [M, 384] hidden tile formed once.
//
// The pair it replaces -- the chain kernel of mlp_fused.hip and the weight-gradient kernel of mlp_wgrad.hip -- both rebuild H = LN(y1) W1 + b1
// and dG = dbr (W2 gamma)^T: 7 products and 3 GELU-family evaluations per hidden element where 5 and 2 are needed, the rows staged, normalised
// and row-scaled four times.  Here a workgroup owns a chunk of rows and ALL 384 hidden units, in the orientation of mlp_wgrad.hip (accumulator:
// lane = hidden unit, registers = rows, which IS the A operand of the two row contractions):
//     per 32-row tile and wavefront (48 hidden units = 3 groups of 16):
//         H, dG          16x16x32 MFMA: A = y / dbr rows (LDS tile), B = W1 fragments (LDS image) / W2 gamma fragments (global, L1-resident)
//         G, gelu'       gelu_sig_both, ONE evaluation;  dH = dG o gelu' rounded to bf16
//         Z += G^T dbr,  dW1T += dH^T y,  db1 += colsum(dH)      accumulators in registers over the whole chunk (144 per lane)
//         dH -> LDS [32 rows][384] (the only tensor that changes orientation)
//     barrier;  dy2 = dH W1^T: twelve 16 x 16 output tiles over the eight wavefronts, each over the full K = 384 -- A = dH rows (two
//         ds_read_b64 in the transposed fragment's k order), B = ds_read_b64_tr_b16 of the SAME W1 image ([hid][c] rows serve the H product
//         row-wise and this one column-wise);  dy2 -> fp32 LDS tile (it takes the place of the y | d tile just consumed)
//     barrier;  LayerNorm backward on the tile (the arithmetic of the LNB epilogue of mlp_fused.hip = layernorm_bwd_kernel): a 32-lane half owns
//         a row (3 channels per lane), row sums by xor-shuffles, dy1 stored, dgamma | dbeta column sums kept in registers over the chunk.
// No atomics: the chunk records [Z | dW1T | db1 | S] are summed by the fixed-order row reduction and booked by the finish launch of
// mlp_wgrad_common.h, the LayerNorm column sums leave as one partial row per chunk for the (deferred) fixed-order reduction.
//
// LDS (161152 of 163840 bytes): y | d tiles, double-buffered, 36864; W1 image [384][96 + 16] 86016 (224-byte rows: conflict-free for the
// ds_read_b128 groups -- slot (-2 row + k-quarter) mod 16 -- and for the transposed reads, 8 rows x 32 bytes at 56-dword steps); dH tile
// [32][384 + 8] 25088; raw y1 rows for xhat, double-buffered, 12288; mean | rstd of the rows 512; ln_gamma 384.  W2 gamma does not fit beside W1: its B
// fragments (9 x 16 bytes per lane and tile) are read from the tiled image in global memory, which stays in L1 / L2.
// Registers: 144 accumulators + 3 db1 + 9 column sums (S, dgamma, dbeta of the LayerNorm) + 10 of the next tile's rows + 13 of the next
// hidden group's W2 gamma fragments and bias + the fragment windows = 250 of the 256 that two wavefronts per SIMD have (no scratch).
// The next tile's global loads are issued at the head of the hidden phase and committed to LDS after the LayerNorm epilogue; the W2 gamma
// fragments are requested one hidden group ahead.
//
// Measured (MI355X, stage 0: M = 262144): 253 us with the record reduction (256 x 297 KB) and the finish launch, against 148 + 174 us for the
// pair (tools/kbench_mlp_bwd_onepass.py; profiles/mlp_bwd_onepass_ab.md).
#include "common.h"
#include "iseg_hip.h"
#include "mlp_common.h"
#include "mlp_wgrad_common.h"

namespace {

struct OpGeom {
    static constexpr int C = 96, HID = 4 * C, WAVES = 8, NT = 64 * WAVES, RT = 32, KS = C / 32, CBS = C / 16;
    static constexpr int NG = HID / (16 * WAVES);                  // hidden groups of 16 per wavefront
    static constexpr int YSTR = 144, TILE = RT * YSTR;             // y | d tiles: 288-byte rows (mlp_wgrad.hip)
    static constexpr int WSTR = 112;                               // W1 image [hid][c]: 224-byte rows
    static constexpr int HSTR = HID + 8;                           // dH tile: 784-byte rows (49 x 16: a ds_read_b64 half touches 64 banks once)
    static constexpr int DSTR = C + 4;                             // dy2 fp32 tile
    static constexpr int CPR = C / 8, NLOAD = CPR * RT;            // staging: 16-byte chunks per row, loader threads (one row each)
    static constexpr int OFF_W1 = 2 * 2 * TILE * 2;
    static constexpr int OFF_DH = OFF_W1 + HID * WSTR * 2;
    static constexpr int OFF_RAW = OFF_DH + RT * HSTR * 2;
    static constexpr int OFF_ST = OFF_RAW + 2 * RT * C * 2;
    static constexpr int OFF_LG = OFF_ST + 2 * RT * 2 * 4;
    static constexpr int LDS = OFF_LG + C * 4;
    static constexpr int IMG = C * 64, SLAB = 3 * IMG;             // tiled backward weight buffer of mlp_fused.hip: [slab][A1 | A3 | A4]
    static constexpr int64_t REC = mlp_record_floats(C);           // chunk record [Z | dW1T | db1 | S]
    static_assert(NG == 3 && NLOAD <= NT && RT * DSTR * 4 <= 2 * TILE * 2 && 3 * (NT / 32) * C * 4 <= RT * HSTR * 2 && LDS <= 160 * 1024,
                  "geometry");
};

__global__ __launch_bounds__(512) void convnext_mlp_bwd_onepass_kernel(const bf16_t* __restrict__ Y, const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd, const float* __restrict__ ln_gamma,
                                                                       const float* __restrict__ ln_beta, const bf16_t* __restrict__ D,
                                                                       const float* __restrict__ rowscale, int64_t rows_per_group,
                                                                       const void* __restrict__ BW, const float* __restrict__ b1,
                                                                       bf16_t* __restrict__ DY, float* __restrict__ part,
                                                                       float* __restrict__ lnpart, int64_t M, int64_t rows_per_chunk) {
    using G = OpGeom;
    constexpr int C = G::C, HID = G::HID, KS = G::KS, CBS = G::CBS, NG = G::NG, RT = G::RT, CPR = G::CPR;
    constexpr int YSTR = G::YSTR, TILE = G::TILE, WSTR = G::WSTR, HSTR = G::HSTR, DSTR = G::DSTR;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* const tiles = reinterpret_cast<bf16_t*>(smem);                    // [buf][y | d][RT][YSTR]
    bf16_t* const w1img = reinterpret_cast<bf16_t*>(smem + G::OFF_W1);        // [HID][WSTR]
    bf16_t* const dht = reinterpret_cast<bf16_t*>(smem + G::OFF_DH);          // [RT][HSTR]
    bf16_t* const raws = reinterpret_cast<bf16_t*>(smem + G::OFF_RAW);        // [buf][RT][C]
    float* const stats = reinterpret_cast<float*>(smem + G::OFF_ST);          // [buf][RT][mean | rstd]
    float* const lgs = reinterpret_cast<float*>(smem + G::OFF_LG);            // ln_gamma

    const int chunk = blockIdx.x;
    const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // (scalar: the hidden groups' offsets stay out of the VGPRs)
    // REGISTERS.  The 144 accumulators leave ~100 registers for everything else, and hipcc hoists every loop-invariant lane address (LDS bases
    // of each hidden group and phase, global row offsets, the per-tile re-reads of W2 gamma / b1 / ln_gamma) out of the tile loop: 60 + 55
    // registers held for the whole kernel, the accumulators spilled around their MFMAs.  So each phase derives its addresses from a thread id
    // the compiler cannot see through: a few integer instructions per phase instead of a register each.
    auto opaque = [](int v) {
        asm volatile("" : "+v"(v));
        return v;
    };
    const int64_t r_begin = (int64_t)chunk * rows_per_chunk;
    const int64_t r_end = r_begin + rows_per_chunk < M ? r_begin + rows_per_chunk : M;
    const int ntiles = (int)((r_end - r_begin + RT - 1) / RT);

    // ---- W1 image [hid][c] from the A1 pieces of the tiled buffer (piece kk of slab s: [k-half][32 hid][8 c], 16-byte fragments) ----
    for (int i = tid; i < HID * CPR; i += G::NT) {
        const int hid = i / CPR, c8 = i % CPR;
        const char* src = (const char*)BW + (int64_t)(hid >> 5) * G::SLAB + (c8 >> 1) * 1024 + mlp_frag_offset(hid & 31, c8 & 1);
        *reinterpret_cast<bf16x8*>(w1img + hid * WSTR + 8 * c8) = *reinterpret_cast<const bf16x8*>(src);
    }
    if (tid < C) lgs[tid] = ln_gamma[tid];

    // ---- staging role: thread -> (row of the tile, 16-byte chunk of the row); one row of the tile each ----
    // (threads past NLOAD load row 0 again and drop it)
    bf16x8 ry, rd;
    float rmean, rrstd;
    bool rok;
    // Global loads of tile t into registers.  No branch: past the last tile the loads repeat the last tile's addresses and the row is flagged
    // invalid (mlp_wgrad.hip: with a branch around issue() and commit() hipcc sinks the loads into the commit block).
    auto issue = [&](int t) {
        const int tq = opaque(tid);
        const bool loader = tq < G::NLOAD;
        const int cpos = tq % CPR, rg = loader ? tq / CPR : 0;
        const bool live = t < ntiles;
        const int tt = live ? t : ntiles - 1;
        const int64_t row = r_begin + (int64_t)tt * RT + rg;
        const int64_t rr = row < r_end ? row : r_begin;
        ry = *reinterpret_cast<const bf16x8*>(Y + rr * C + 8 * cpos);
        rd = *reinterpret_cast<const bf16x8*>(D + rr * C + 8 * cpos);
        rmean = mean[rr];
        rrstd = rstd[rr];
        rok = live && loader && row < r_end;
    };
    auto commit = [&](int t, int buf) {      // registers -> LDS: LayerNorm(y1), dbr = row factor x dout, raw y1 and the statistics
        const int tq = opaque(tid);
        const bool loader = tq < G::NLOAD;
        const int cpos = tq % CPR, rg = loader ? tq / CPR : 0;
        const int64_t row0 = r_begin + (int64_t)(t < ntiles ? t : ntiles - 1) * RT;
        const float rs = rowscale ? rowscale[row0 / rows_per_group] : 1.f;
        float lg[8], lb[8];
        const int cp = 8 * cpos;
        load8<float>(ln_gamma + cp, lg);
        load8<float>(ln_beta + cp, lb);
        bf16x8 yr = ry, y = ry, d = rd;
        float mu = rmean, rsd = rrstd;
        if (!rok) {      // rows past the chunk: zero dbr (no contribution anywhere), y2 = 0, xhat = 0
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                yr[u] = (bf16_t)0.f;
                y[u] = (bf16_t)0.f;
                d[u] = (bf16_t)0.f;
            }
            mu = 0.f;
            rsd = 0.f;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) y[u] = (bf16_t)iseg_ln_apply((float)y[u], mu, rsd, lg[u], lb[u]);
        }
        if (rowscale) {
#pragma unroll
            for (int u = 0; u < 8; ++u) d[u] = (bf16_t)((float)d[u] * rs);
        }
        if (loader) {
            *reinterpret_cast<bf16x8*>(tiles + (buf * 2 + 0) * TILE + rg * YSTR + 8 * cpos) = y;
            *reinterpret_cast<bf16x8*>(tiles + (buf * 2 + 1) * TILE + rg * YSTR + 8 * cpos) = d;
            *reinterpret_cast<bf16x8*>(raws + (buf * RT + rg) * C + 8 * cpos) = yr;
            if (cpos == 0) {
                stats[(buf * RT + rg) * 2] = mu;
                stats[(buf * RT + rg) * 2 + 1] = rsd;
            }
        }
    };

    f32x4 zacc[NG][CBS], wacc[NG][CBS];
    float db1[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        db1[g] = 0.f;
#pragma unroll
        for (int cb = 0; cb < CBS; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) zacc[g][cb][r] = wacc[g][cb][r] = 0.f;
    }

    // ---- LayerNorm-backward role: 32-lane half hw owns rows hw and hw + 16 of a tile, lane j the channels j, j + 32, j + 64 ----
    float cgs[3], cbs[3], ssum[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) cgs[i] = cbs[i] = ssum[i] = 0.f;

    // Hidden-tile phase of one 32-row tile.  Order pinned by sched_barrier as in mlp_wgrad.hip: the fragments of a k-step are requested in one
    // batch in front of its MFMAs (no room for a second batch in flight), the transposed B fragments of the row contractions inside the gelu
    // section that covers their latency.
    constexpr int CG = 2;
    // W2 gamma fragments and b1 of hidden group hg: requested one group ahead (behind the MFMAs that read the previous group's, whose registers
    // they take over), the first group of the NEXT tile behind the last group of this one, so that the L1 / L2 round trip is never waited for
    bf16x8 w3f[KS];
    float bias;
    auto fetch_w3 = [&](int hg) {
        const int lane = opaque(tid) & 63, li = lane & 15, q = lane >> 4;
        const char* p = (const char*)BW + (hg >> 1) * G::SLAB + (hg & 1) * 256 + G::IMG + (q >> 1) * 1024 + mlp_frag_offset(li, q & 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) w3f[ks] = *reinterpret_cast<const bf16x8*>(p + ks * 2048);
        bias = b1[hg * 16 + li];
    };
    fetch_w3(wid * NG);
    auto hidden = [&](int t, int buf) {
        const bf16_t* const ty = tiles + (buf * 2 + 0) * TILE;
        const bf16_t* const td = tiles + (buf * 2 + 1) * TILE;
        issue(t + 1);      // (a whole hidden phase ahead of its commit: HBM latency; the W2 gamma requests behind it wait a group later, when it has landed)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int hg = wid * NG + g, hid0 = hg * 16;      // this wavefront's g-th group of 16 hidden units
            const int lane = opaque(tid) & 63, li = lane & 15, q = lane >> 4;
            f32x4 hacc[2], dacc[2];
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    hacc[b][r] = bias;
                    dacc[b][r] = 0.f;
                }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 ay[2], ad[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int o = (b * 16 + li) * YSTR + 32 * ks + 8 * q;
                    ay[b] = *reinterpret_cast<const bf16x8*>(ty + o);
                    ad[b] = *reinterpret_cast<const bf16x8*>(td + o);
                }
                const bf16x8 w1f = *reinterpret_cast<const bf16x8*>(w1img + (hid0 + li) * WSTR + 32 * ks + 8 * q);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    hacc[b] = mfma16(ay[b], w1f, hacc[b]);
                    dacc[b] = mfma16(ad[b], w3f[ks], dacc[b]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            fetch_w3(wid * NG + (g + 1) % NG);
            __builtin_amdgcn_sched_barrier(0);
            // gelu in two batches of four (left in one region the scheduler interleaves all eight evaluations: 40 registers of temporaries);
            // the transposed fragments are requested between them
            bf16x8 bd[CG], by[CG], gf, hf;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float gl, gd;
                    gelu_sig_both(hacc[b][r], gl, gd);
                    const bf16_t dh = (bf16_t)(dacc[b][r] * gd);
                    gf[4 * b + r] = (bf16_t)gl;
                    hf[4 * b + r] = dh;
                    db1[g] += (float)dh;
                    dht[(16 * b + 4 * q + r) * HSTR + hid0 + li] = dh;
                }
                asm volatile("" : "+v"(db1[g]));      // (or the adds sink to the end of the tile loop and all 24 dH values stay live)
                __builtin_amdgcn_sched_barrier(0);
                if (b == 0) {
#pragma unroll
                    for (int c = 0; c < CG; ++c) {
                        bd[c] = tr_frag(td, YSTR, c, lane);
                        by[c] = tr_frag(ty, YSTR, c, lane);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int c0 = 0; c0 < CBS; c0 += CG) {
                if (c0 > 0) {
#pragma unroll
                    for (int c = 0; c < CG; ++c) {
                        bd[c] = tr_frag(td, YSTR, c0 + c, lane);
                        by[c] = tr_frag(ty, YSTR, c0 + c, lane);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int c = 0; c < CG; ++c) {
                    zacc[g][c0 + c] = mfma16(gf, bd[c], zacc[g][c0 + c]);
                    wacc[g][c0 + c] = mfma16(hf, by[c], wacc[g][c0 + c]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // S = column sums of dbr, in the LayerNorm role (the d tile makes way for dy2 behind the next barrier)
        const int tq = opaque(tid), hw = tq >> 5, j32 = tq & 31;
#pragma unroll
        for (int ps = 0; ps < 2; ++ps)
#pragma unroll
            for (int i = 0; i < 3; ++i) ssum[i] += (float)td[(hw + 16 * ps) * YSTR + j32 + 32 * i];
    };

    // dy2 tile (16 rows mt, 16 channels ct) = dH rows . W1^T over all 384 hidden units -> fp32 LDS tile.  The transposed read hands the k
    // slots out as hidden units 4 q + j (j < 4), 16 + 4 q + j - 4 of each 32-unit step: the A fragment is gathered in that order.
    auto dy2_tile = [&](int tile, float* dyt) {
        const int mt = tile & 1, ct = tile >> 1;
        const int lane = opaque(tid) & 63, li = lane & 15, q = lane >> 4;
        f32x4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = 0.f;
        const bf16_t* const arow = dht + (16 * mt + li) * HSTR + 4 * q;
#pragma unroll
        for (int ks = 0; ks < HID / 32; ++ks) {
            const bf16x4 lo = *reinterpret_cast<const bf16x4*>(arow + 32 * ks);
            const bf16x4 hi = *reinterpret_cast<const bf16x4*>(arow + 32 * ks + 16);
            bf16x8 a;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = lo[i];
                a[4 + i] = hi[i];
            }
            acc = mfma16(a, tr_frag(w1img + 32 * ks * WSTR, WSTR, ct, lane), acc);
            if (ks % 4 == 3) __builtin_amdgcn_sched_barrier(0);      // (four k-steps of fragments in flight, not all twelve: registers)
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dyt[(16 * mt + 4 * q + r) * DSTR + 16 * ct + li] = acc[r];
    };

    // LayerNorm backward of the tile's rows (keras LayerNormalization; layernorm_bwd_kernel of norm.hip):
    //   t = dy2 * gamma,  dy1 = rstd * (t - mean_c(t) - xhat * mean_c(t * xhat)),  dgamma += dy2 * xhat,  dbeta += dy2   (column sums)
    auto layernorm_bwd = [&](int t, int buf, const float* dyt) {
        const int64_t row0 = r_begin + (int64_t)t * RT;
        const int tq = opaque(tid), hw = tq >> 5, j32 = tq & 31;
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int rr = hw + 16 * ps;
            const float mu = stats[(buf * RT + rr) * 2], rsd = stats[(buf * RT + rr) * 2 + 1];
            float v[3], xh[3], tt[3];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v[i] = dyt[rr * DSTR + j32 + 32 * i];
                xh[i] = ((float)raws[(buf * RT + rr) * C + j32 + 32 * i] - mu) * rsd;
                tt[i] = v[i] * lgs[j32 + 32 * i];
                s1 += tt[i];
                s2 = fmaf(tt[i], xh[i], s2);
            }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {      // the 32 lanes of the row (fixed order: bit-reproducible)
                s1 += __shfl_xor(s1, o);
                s2 += __shfl_xor(s2, o);
            }
            s1 *= 1.f / (float)C;
            s2 *= 1.f / (float)C;
            const int64_t row = row0 + rr;
            if (row < r_end) {
#pragma unroll
                for (int i = 0; i < 3; ++i) DY[row * C + j32 + 32 * i] = (bf16_t)(rsd * (tt[i] - s1 - xh[i] * s2));
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {      // (rows past the chunk: dy2 = 0)
                cgs[i] = fmaf(v[i], xh[i], cgs[i]);
                cbs[i] += v[i];
            }
        }
    };

    issue(0);
    commit(0, 0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        hidden(t, buf);
        __syncthreads();      // the dH tile is complete, every wavefront is past its reads of the y | d tile
        float* const dyt = reinterpret_cast<float*>(tiles + buf * 2 * TILE);
        dy2_tile(wid, dyt);
        if (wid < 4) dy2_tile(8 + wid, dyt);      // (wave-uniform: the transposed reads see a full EXEC mask)
        __syncthreads();
        layernorm_bwd(t, buf, dyt);
        commit(t + 1, buf ^ 1);
        __syncthreads();
    }

    // ---- partial results of this chunk: [Z | dW1T | db1 | S] ----
    const int lane = tid & 63, li = lane & 15, q = lane >> 4, hw = tid >> 5, j32 = tid & 31;
    float* const pz = part + (int64_t)chunk * G::REC;
    float* const pw = pz + (int64_t)HID * C;
    float* const pb = pw + (int64_t)HID * C;
    float* const ps = pb + HID;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int hid0 = (wid * NG + g) * 16;
#pragma unroll
        for (int cb = 0; cb < CBS; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t o = (int64_t)(hid0 + 4 * q + r) * C + 16 * cb + li;
                pz[o] = zacc[g][cb][r];
                pw[o] = wacc[g][cb][r];
            }
        // the four lanes li, li + 16, li + 32, li + 48 hold the same hidden unit
        unsigned u = __builtin_bit_cast(unsigned, db1[g]);
        auto sw = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        float v = __builtin_bit_cast(float, (unsigned)sw[0]) + __builtin_bit_cast(float, (unsigned)sw[1]);
        u = __builtin_bit_cast(unsigned, v);
        auto sx = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        v = __builtin_bit_cast(float, (unsigned)sx[0]) + __builtin_bit_cast(float, (unsigned)sx[1]);
        if (lane < 16) pb[hid0 + li] = v;
    }
    // S and the LayerNorm column sums: registers -> LDS (the dH tile: the loop ended on a barrier) -> one value per channel, in fixed order
    float* const ls = reinterpret_cast<float*>(smem + G::OFF_DH);      // [NT / 32][S | dgamma | dbeta]
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ls[hw * 3 * C + j32 + 32 * i] = ssum[i];
        ls[hw * 3 * C + C + j32 + 32 * i] = cgs[i];
        ls[hw * 3 * C + 2 * C + j32 + 32 * i] = cbs[i];
    }
    __syncthreads();
    if (tid < 3 * C) {
        float v = 0.f;
        for (int g = 0; g < G::NT / 32; ++g) v += ls[g * 3 * C + tid];
        if (tid < C) ps[tid] = v;
        else lnpart[(int64_t)chunk * 2 * C + tid - C] = v;
    }
}

}  // namespace

extern "C" int iseg_convnext_mlp_bwd_onepass(const void* y1, const float* mean, const float* rstd, const float* ln_gamma, const float* ln_beta,
                                             const void* dout, const float* rowscale, int64_t rows_per_group, const void* bw_tiled,
                                             const float* b1, const float* W2, const float* b2, const float* gamma, void* dy1,
                                             float* dln_gamma, float* dln_beta, float* dW1, float* db1, float* dW2, float* db2, float* dgamma,
                                             int64_t M, int C, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
    using G = OpGeom;
    ISEG_REQUIRE(dtype == ISEG_BF16 && C == 96, "iseg_convnext_mlp_bwd_onepass: bf16 storage with C = 96 only (C = %d, dtype = %d)", C, dtype);
    ISEG_REQUIRE(y1 && mean && rstd && ln_gamma && ln_beta && dout && bw_tiled && b1 && W2 && b2 && dy1 && dln_gamma && dln_beta && dW1 && db1 &&
                     dW2 && db2 && M > 0, "iseg_convnext_mlp_bwd_onepass: null operand or empty problem");
    ISEG_REQUIRE(!gamma || dgamma, "iseg_convnext_mlp_bwd_onepass: gamma needs dgamma");
    ISEG_REQUIRE(!rowscale || (rows_per_group > 0 && rows_per_group % 64 == 0),
                 "iseg_convnext_mlp_bwd_onepass: the row factor must be constant inside 64-row tiles (rows_per_group = %lld)", (long long)rows_per_group);
    ISEG_REQUIRE((((uintptr_t)y1 | (uintptr_t)dout | (uintptr_t)bw_tiled | (uintptr_t)ln_gamma | (uintptr_t)ln_beta | (uintptr_t)dy1) & 15) == 0,
                 "iseg_convnext_mlp_bwd_onepass: operands must be 16-byte aligned");
    // (sized by the weight-gradient pair's function: one answer for both launchers that leave these chunk records, mlp_wgrad_common.h)
    const size_t need = iseg_convnext_mlp_wgrad_workspace_bytes(M, C);
    ISEG_NEED_WORKSPACE("iseg_convnext_mlp_bwd_onepass", ws, ws_bytes, need);
    int nchunk;
    const int rpc = onepass_rows_per_chunk(M, &nchunk);
    const MlpGradWs L = onepass_ws(M);
    float* const wsf = (float*)ws;
    // dln_gamma | dln_beta: one partial row per chunk, summed in fixed order into the gradient buffers (queued when the caller defers reductions)
    RowReduce ln_red{.P = nchunk, .pstride = 2 * G::C, .n = 2 * G::C, .out0 = dln_gamma, .out1 = dln_beta, .n0 = G::C, .accumulate = 1};
    float* const lnpart = reduce_rows_begin(ln_red, L.lnpart(wsf), stream);
    static const bool raised = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&convnext_mlp_bwd_onepass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   G::LDS) == hipSuccess;
    }();
    (void)raised;
    hipLaunchKernelGGL(convnext_mlp_bwd_onepass_kernel, dim3(nchunk), dim3(G::NT), G::LDS, stream, (const bf16_t*)y1, mean, rstd, ln_gamma, ln_beta,
                       (const bf16_t*)dout, rowscale, rows_per_group, bw_tiled, b1, (bf16_t*)dy1, L.records(wsf), lnpart, M, (int64_t)rpc);
    const int rc = iseg_check_launch("iseg_convnext_mlp_bwd_onepass");
    if (rc != ISEG_OK) return rc;
    reduce_rows_end(ln_red, stream);
    // chunk records -> their sum -> the parameter gradients (mlp_wgrad_common.h)
    return mlp_grads_from_records(L, wsf, W2, b2, gamma, dW1, db1, dW2, db2, dgamma, "iseg_convnext_mlp_bwd_onepass_finish", stream);
}
