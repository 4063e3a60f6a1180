// Patchify convolutions -- kernel == stride, no dilation, one group, H % KH == 0 and W % KW == 0, so "same" padding pads nothing
// (backbones/convnext.py:72-75: the 2x2 / stride-2 downsampling layers) -- as plain GEMMs over a PATCH VIEW of the NHWC tensor.
//
// The patch matrix P[r, (a, j)], r = (n*Ho + oh)*Wo + ow, a < KH, j < KW*C, is the tensor itself read at
//     x + (r / Wo) * (KH*W*C) + (r % Wo) * (KW*C) + a * (W*C) + j
// rows with a grouped stride (a jump every Wo rows), K made of KH contiguous segments of KW*C elements.  No copy is needed to read or write it:
//   forward          y  = P W + b      gemm_bf16_dma_kernel<PV = 1>: only the per-lane DMA source address of the A pieces changes
//   data gradient    dx = dy W^T       gemm_bf16_dma_kernel<PV = 2>: the same product as the column-buffer route (same tile form, same summation
//                                      order: bit-identical), its 16-byte vectors stored at the patch address -- no column buffer, no col2im
//   weight gradient  dW (+)= P^T dy    gemm_bf16_dma_tn_kernel's loop with P as the [K rows][M columns] operand, the split rule, fp32 slabs and
//                                      fixed-order slab sum of iseg_gemm; the bias gradient rides its ones-row
// The tile forms, their selection and the split rule are those of iseg_gemm for the same M, N, K (gemm_dma.h, gemm_dma_tn.h).
#include "common.h"
#include "iseg_hip.h"

#include "gemm_dma_tn.h"

using namespace iseg_mm;

namespace {

const void* const ALIGNED = reinterpret_cast<const void*>(uintptr_t(4096));      // stands for an operand in the geometry-only queries

bool patch_geom_ok(const iseg_conv_geom* g, int dtype) {
    if (!g || dtype != ISEG_BF16) return false;
    if (g->N <= 0 || g->H <= 0 || g->W <= 0 || g->Cin <= 0 || g->Cout <= 0 || g->KH <= 0 || g->KW <= 0 || g->groups != 1) return false;
    if (g->sh != g->KH || g->sw != g->KW || g->dh != 1 || g->dw != 1 || g->pt != 0 || g->pl != 0) return false;
    if (g->H % g->KH != 0 || g->W % g->KW != 0 || g->Ho != g->H / g->KH || g->Wo != g->W / g->KW) return false;
    // 16-byte vectors stay inside one segment; row and column indices are ints in the kernels
    if (((int64_t)g->KW * g->Cin) % 8 != 0 || g->Cout % 8 != 0) return false;
    if ((int64_t)g->N * g->H * g->W * g->Cin >= (1ll << 31) || (int64_t)g->N * g->Ho * g->Wo * g->Cout >= (1ll << 31)) return false;
    return true;
}

int64_t rows_of(const iseg_conv_geom* g) { return (int64_t)g->N * g->Ho * g->Wo; }
int64_t kd_of(const iseg_conv_geom* g) { return (int64_t)g->KH * g->KW * g->Cin; }

void set_view(Epi& e, const iseg_conv_geom* g) {
    e.pv_wo = g->Wo;
    e.pv_seg = g->KW * g->Cin;
    e.pv_segstride = (int64_t)g->W * g->Cin;
    e.pv_group = (int64_t)g->KH * g->W * g->Cin;
}

// the GEMM each pass is, in iseg_gemm's terms (the patch-view operand gets the row stride of the column buffer it stands for)
iseg_gemm_args fwd_args(const void* x, const void* wt, const float* bias, void* y, const iseg_conv_geom* g) {
    iseg_gemm_args a{};
    a.A = x, a.lda = kd_of(g), a.a_kcontig = 1;
    a.B = wt, a.ldb = kd_of(g), a.b_kcontig = 1;
    a.D = y, a.ldd = g->Cout;
    a.M = rows_of(g), a.N = g->Cout, a.K = kd_of(g);
    a.in_dtype = a.out_dtype = ISEG_BF16;
    a.bias = bias;
    a.alpha = 1.f;
    return a;
}

iseg_gemm_args dgrad_args(const void* dy, const void* w, void* dx, const iseg_conv_geom* g) {
    iseg_gemm_args a{};
    a.A = dy, a.lda = g->Cout, a.a_kcontig = 1;
    a.B = w, a.ldb = g->Cout, a.b_kcontig = 1;      // the Keras kernel [KH*KW*Cin][Cout] is K-contiguous for this product
    a.D = dx, a.ldd = kd_of(g);
    a.M = rows_of(g), a.N = kd_of(g), a.K = g->Cout;
    a.in_dtype = a.out_dtype = ISEG_BF16;
    a.alpha = 1.f;
    return a;
}

iseg_gemm_args wgrad_args(const void* x, const void* dy, float* dw, float* dbias, int accumulate, const iseg_conv_geom* g) {
    iseg_gemm_args a{};
    a.A = x, a.lda = kd_of(g), a.a_kcontig = 0;
    a.B = dy, a.ldb = g->Cout, a.b_kcontig = 0;
    a.D = dw, a.ldd = g->Cout;
    a.M = kd_of(g), a.N = g->Cout, a.K = rows_of(g);
    a.in_dtype = ISEG_BF16, a.out_dtype = ISEG_F32;
    a.alpha = 1.f;
    a.accumulate = accumulate;
    a.colsum_out = dbias;
    a.colsum_accumulate = accumulate;
    return a;
}

bool fwd_ok(const iseg_gemm_args& a, const iseg_conv_geom* g) {
    if (!dma_eligible(&a, a.K, false) || iseg_gemm_splits(&a) != 1) return false;
    return ((int64_t)g->KW * g->Cin) % dma_kstep(&a) == 0;      // no K-step straddles two segments
}

bool dgrad_ok(const iseg_gemm_args& a) { return dma_eligible(&a, a.K, false) && iseg_gemm_splits(&a) == 1; }

// the weight-gradient LDS-DMA form (7 / 8) the problem takes with the split iseg_gemm chooses, 0 = not this route
int wgrad_form(const iseg_gemm_args& a) {
    const int form = dma_tn_form(&a);
    return form && dma_tn_split(&a, form) > 1 ? form : 0;
}

}  // namespace

namespace iseg_mm {
// iseg_conv2d_igemm_workspace_bytes(geom, 3): the slabs of the patch-view weight gradient (with the ones-row of the bias gradient)
size_t conv_patch_wgrad_workspace(const iseg_conv_geom* g) {
    if (!patch_geom_ok(g, ISEG_BF16)) return 0;
    iseg_gemm_args a = wgrad_args(ALIGNED, ALIGNED, (float*)ALIGNED, (float*)ALIGNED, 1, g);
    if (!wgrad_form(a)) return 0;
    return iseg_gemm_workspace_bytes(&a);
}
}  // namespace iseg_mm

extern "C" int iseg_conv2d_patch_supported(const iseg_conv_geom* g, int dtype, int pass) {
    if (!patch_geom_ok(g, dtype)) return 0;
    if (pass == 0) return fwd_ok(fwd_args(ALIGNED, ALIGNED, nullptr, const_cast<void*>(ALIGNED), g), g) ? 1 : 0;
    if (pass == 1) return dgrad_ok(dgrad_args(ALIGNED, ALIGNED, const_cast<void*>(ALIGNED), g)) ? 1 : 0;
    if (pass == 2) return wgrad_form(wgrad_args(ALIGNED, ALIGNED, (float*)ALIGNED, (float*)ALIGNED, 1, g)) ? 1 : 0;
    return 0;
}

extern "C" int iseg_conv2d_patch_fwd(const void* x, const void* wt, const float* bias, void* y, const iseg_conv_geom* g, int dtype, void* ws,
                                     size_t ws_bytes, hipStream_t stream) {
    (void)ws, (void)ws_bytes;      // (never split: no scratch)
    ISEG_REQUIRE(x && wt && y, "iseg_conv2d_patch_fwd: null operand");
    const iseg_gemm_args a = patch_geom_ok(g, dtype) ? fwd_args(x, wt, bias, y, g) : iseg_gemm_args{};
    if (!patch_geom_ok(g, dtype) || !fwd_ok(a, g)) {
        iseg_set_error("iseg_conv2d_patch_fwd: not a patchify convolution this route takes (iseg_conv2d_patch_supported(geom, dtype, 0)), or operands not 16-byte aligned");
        return ISEG_ERR_UNSUPPORTED;
    }
    Epi e = plain_epi(bias, 0);
    set_view(e, g);
    if (bias) dispatch_dma_patch<1, EK_BIAS>(&a, e, stream);
    else dispatch_dma_patch<1, EK_PLAIN>(&a, e, stream);
    return iseg_check_launch("iseg_conv2d_patch_fwd");
}

extern "C" int iseg_conv2d_patch_bwd_data(const void* dy, const void* w, void* dx, const iseg_conv_geom* g, int dtype, void* ws, size_t ws_bytes,
                                          hipStream_t stream) {
    (void)ws, (void)ws_bytes;
    ISEG_REQUIRE(dy && w && dx, "iseg_conv2d_patch_bwd_data: null operand");
    const iseg_gemm_args a = patch_geom_ok(g, dtype) ? dgrad_args(dy, w, dx, g) : iseg_gemm_args{};
    if (!patch_geom_ok(g, dtype) || !dgrad_ok(a)) {
        iseg_set_error("iseg_conv2d_patch_bwd_data: not a patchify convolution this route takes (iseg_conv2d_patch_supported(geom, dtype, 1)), or operands not 16-byte aligned");
        return ISEG_ERR_UNSUPPORTED;
    }
    Epi e = plain_epi(nullptr, 0);
    set_view(e, g);
    dispatch_dma_patch<2, EK_PLAIN>(&a, e, stream);
    return iseg_check_launch("iseg_conv2d_patch_bwd_data");
}

extern "C" int iseg_conv2d_patch_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int accumulate, const iseg_conv_geom* g, int dtype,
                                            void* ws, size_t ws_bytes, hipStream_t stream) {
    ISEG_REQUIRE(x && dy && dw, "iseg_conv2d_patch_bwd_weight: null operand");
    const iseg_gemm_args a = patch_geom_ok(g, dtype) ? wgrad_args(x, dy, dw, dbias, accumulate, g) : iseg_gemm_args{};
    const int form = patch_geom_ok(g, dtype) ? wgrad_form(a) : 0;
    if (!form || ((uintptr_t)dw % 16) || (dbias && (uintptr_t)dbias % 16)) {
        iseg_set_error("iseg_conv2d_patch_bwd_weight: not a patchify convolution this route takes (iseg_conv2d_patch_supported(geom, dtype, 2)), or operands not 16-byte aligned");
        return ISEG_ERR_UNSUPPORTED;
    }
    const SplitPlan plan = split_plan(a.K, iseg_gemm_splits(&a), 128, a.M + (dbias ? 1 : 0), a.N);      // iseg_gemm's plan for the same M, N, K
    ISEG_NEED_WORKSPACE("iseg_conv2d_patch_bwd_weight", ws, ws_bytes, plan.slab_bytes);
    TnPatch pv{g->Wo, g->KW * g->Cin, (int64_t)g->KH * g->W * g->Cin, (int64_t)g->W * g->Cin, 0};
    if (64 % g->Wo == 0) pv.adv = (int64_t)(64 / g->Wo) * pv.group;      // 64 reduction rows = whole pixel rows: a constant per-stage advance
    if (form == 7) launch_dma_tn_patch<4, 2>(&a, pv, plan.eff_split, plan.kps, (float*)ws, stream);
    else launch_dma_tn_patch<2, 4>(&a, pv, plan.eff_split, plan.kps, (float*)ws, stream);
    Epi e = plain_epi(nullptr, accumulate);
    e.colsum_out = dbias, e.colsum_accumulate = accumulate;
    return gemm_reduce(e, dw, a.ldd, ISEG_F32, a.M, a.N, (float*)ws, plan, stream);
}
